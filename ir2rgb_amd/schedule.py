"""What the reference does between windows and between epochs, as plain host arithmetic (no torch, no device).

    linear learning-rate decay            models/models.py:112-116, base_model.py:94-99
    sequence-length growth                models/models.py:118-121, data/dataset/vid2vid.py:99-107
    frames per window / per backward      base_model.py:109-120 from generator.py:52-56
    finest-scale-only epochs              models/models.py:123-125, generator.py:64-72
    step accounting, save points          train_vid2vid.py:37-151, models/models.py:96-110
    resume                                models/models.py:62-78, :88-90

One process per GPU: the reference's ``n_gpus`` is 1 throughout, its batch size is 1.  ``ir2rgb_amd.training.fit``
drives a trainer with this; everything here can be checked on a CPU (tests/test_schedule_cpu.py).
"""
import math

DEFAULTS = dict(  # options/train_options.py
    niter=10, niter_decay=10, niter_step=5, niter_fix_global=0, n_frames_total=30, max_frames_per_gpu=1,
    max_frames_backpropagate=1, n_input_gen_frames=3, n_scales_spatial=1, lr=2e-4, print_freq=100,
    save_latest_freq=1000, save_epoch_freq=1, seq_len_max=128)


class ScheduleState:
    """What a run holds at the start of an epoch (``TrainingSchedule.start``) and between its sequences."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def training_state(self):
        """The part a resume has to reproduce: (lr, n_frames_total, n_frames_load, n_frames_bp, fix_global)."""
        return (self.lr, self.n_frames_total, self.n_frames_load, self.n_frames_bp, self.fix_global)

    def __repr__(self):
        return "ScheduleState(" + ", ".join(f"{k}={v!r}" for k, v in sorted(self.__dict__.items())) + ")"


class TrainingSchedule:
    def __init__(self, **options):
        unknown = set(options) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"TrainingSchedule: unknown options {sorted(unknown)}")
        o = dict(DEFAULTS)
        o.update(options)
        for k in ("niter", "niter_decay", "niter_fix_global"):
            if not isinstance(o[k], int) or o[k] < 0:
                raise ValueError(f"TrainingSchedule: {k} is a count of epochs, got {o[k]!r}")
        for k in ("niter_step", "n_frames_total", "max_frames_per_gpu", "max_frames_backpropagate", "n_input_gen_frames",
                  "n_scales_spatial", "print_freq", "save_latest_freq", "save_epoch_freq", "seq_len_max"):
            if not isinstance(o[k], int) or o[k] < 1:
                raise ValueError(f"TrainingSchedule: {k} is a positive integer, got {o[k]!r}")
        if o["niter_decay"] == 0 and o["niter"] == 0:
            raise ValueError("TrainingSchedule: niter + niter_decay epochs is an empty run")
        self.opt = o
        self.__dict__.update(o)

    @property
    def last_epoch(self):
        return self.niter + self.niter_decay          # train_vid2vid.py:37

    # ------------------------------------------------------------------ per-epoch rules
    def lr_after(self, epoch):
        """The learning rate in force after the end of ``epoch`` (models.py:114-116, base_model.py:95)."""
        if epoch <= self.niter:
            return self.lr
        return self.lr * (1 - (epoch - self.niter) / self.niter_decay)

    def sequence_cap(self):
        return min(128, self.seq_len_max) - (self.n_input_gen_frames - 1)          # vid2vid.py:104

    def update_sequence_length(self, current, ratio):
        """data/dataset/vid2vid.py:99-107: the dataset's ``current_n_frames_total`` after one call."""
        cap = self.sequence_cap()
        if current < cap:
            current = min(cap, self.n_frames_total * (2 ** ratio))
        return current

    def n_frames_total_after(self, epoch, current=None):
        """Frames per training sequence after the end of ``epoch``; ``current``: the value before it (default: what an
        uninterrupted run holds there).  Grows only at epochs with ``epoch % niter_step == 0`` (models.py:119-120)."""
        if current is None:
            current = self.n_frames_total
            for e in range(self.niter_step, epoch, self.niter_step):
                current = self.update_sequence_length(current, e // self.niter_step)
        if epoch % self.niter_step == 0:
            current = self.update_sequence_length(current, epoch // self.niter_step)
        return current

    def initial_training_batch(self):
        """(n_frames_load, n_frames_bp, n_frames_per_gpu) as the generator is built (generator.py:52-56, n_gpus = 1)."""
        per_gpu = min(self.max_frames_per_gpu, self.n_frames_total)
        return per_gpu, 1, per_gpu

    def update_training_batch(self, n_frames_load, n_frames_bp, n_frames_per_gpu, ratio):
        """One call of Model.update_training_batch (base_model.py:109-120, n_gpus = 1) on the given state."""
        nfb, nfl = n_frames_bp, n_frames_load
        if nfb < nfl:
            nfb = min(self.max_frames_backpropagate, 2 ** ratio)
            n_frames_bp = nfl // int(math.ceil(float(nfl) / nfb))
        if n_frames_per_gpu < self.max_frames_per_gpu:
            n_frames_per_gpu = min(n_frames_per_gpu * 2, self.max_frames_per_gpu)
            n_frames_load = n_frames_per_gpu
        return n_frames_load, n_frames_bp, n_frames_per_gpu

    def training_batch_after(self, ratio):
        """(n_frames_load, n_frames_bp) once the calls for ratios 1..``ratio`` have been made from the initial state: what
        an uninterrupted run holds after epoch ``ratio * niter_step``."""
        state = self.initial_training_batch()
        for r in range(1, ratio + 1):
            state = self.update_training_batch(*state, r)
        return state[0], state[1]

    def fix_global_ends(self, epoch):
        """True at the end of the last finest-scale-only epoch (models.py:124)."""
        return self.n_scales_spatial > 1 and self.niter_fix_global != 0 and epoch == self.niter_fix_global

    def fix_global_at_start(self):
        return self.n_scales_spatial > 1 and self.niter_fix_global != 0            # generator.py:64

    # ------------------------------------------------------------------ a run
    def start(self, n_sequences, start_epoch=1, epoch_iter=0):
        """The state at the start of ``start_epoch``: a fresh run for (1, 0), otherwise what init_params
        (models.py:62-90) sets up from ``iter.txt``.  ``lr_applied`` says whether update_learning_rate has been
        called: the resume calls it for ``start_epoch > niter`` (models.py:70-72), the loop only after epochs
        ``> niter`` (:114-116), so a run resumed at ``niter + 1`` has applied the (still undecayed) rate one epoch before an
        uninterrupted one would."""
        n_load, n_bp, per_gpu = self.initial_training_batch()
        st = ScheduleState(epoch=start_epoch, epoch_iter=epoch_iter, n_sequences=n_sequences, lr=self.lr, lr_applied=False,
                           n_frames_total=self.n_frames_total, n_frames_load=n_load, n_frames_bp=n_bp,
                           n_frames_per_gpu=per_gpu, fix_global=self.fix_global_at_start(), ratio=0)
        if (start_epoch, epoch_iter) != (1, 0):
            if start_epoch > self.niter:
                st.lr, st.lr_applied = self.lr_after(start_epoch - 1), True
            if st.fix_global and start_epoch > self.niter_fix_global:
                st.fix_global = False
            if start_epoch > self.niter_step:
                st.ratio = (start_epoch - 1) // self.niter_step
                st.n_frames_total = self.update_sequence_length(st.n_frames_total, st.ratio)
                # (the reference calls a method its generator does not have here; see training_batch_after)
                st.n_frames_load, st.n_frames_bp = self.training_batch_after(st.ratio)
                st.n_frames_per_gpu = st.n_frames_load
        print_freq = self.print_freq                                               # lcm(print_freq, batch size 1)
        st.total_steps = ((start_epoch - 1) * n_sequences + epoch_iter) // print_freq * print_freq     # models.py:89-90
        return st

    def step(self, st):
        """One sequence of the epoch (train_vid2vid.py:39-44, :119, :139-142).  Advances the counters and returns
        (events, epoch_over): ``events`` a list of ("print", epoch, epoch_iter), ("save_latest", epoch, total_steps,
        (epoch, epoch_iter)) -- the last pair is what ``iter.txt`` then holds."""
        st.total_steps += 1
        st.epoch_iter += 1
        events = []
        if st.total_steps % self.print_freq == 0:
            events.append(("print", st.epoch, st.epoch_iter))
        if st.total_steps % self.save_latest_freq == 0:
            events.append(("save_latest", st.epoch, st.total_steps, (st.epoch, st.epoch_iter)))
        over = st.epoch_iter > st.n_sequences - 1
        if over:
            st.epoch_iter = 0
        return events, over

    def end_epoch(self, st):
        """train_vid2vid.py:149-151 for ``st.epoch``: -> (events, changes).  ``events``: [("save_epoch", epoch, total_steps,
        (epoch + 1, 0))] at a save point; ``changes``: {"lr": ..., "n_frames_total": ..., "training_batch": (n_frames_load,
        n_frames_bp), "update_fixed_params": True} with only the entries that apply.  ``st`` moves to the next epoch."""
        epoch = st.epoch
        events, changes = [], {}
        if epoch % self.save_epoch_freq == 0:
            events.append(("save_epoch", epoch, st.total_steps, (epoch + 1, 0)))
        if epoch > self.niter:
            st.lr, st.lr_applied = self.lr_after(epoch), True
            changes["lr"] = st.lr
        if epoch % self.niter_step == 0:
            st.ratio = epoch // self.niter_step
            st.n_frames_total = self.update_sequence_length(st.n_frames_total, st.ratio)
            st.n_frames_load, st.n_frames_bp, st.n_frames_per_gpu = self.update_training_batch(
                st.n_frames_load, st.n_frames_bp, st.n_frames_per_gpu, st.ratio)
            changes["n_frames_total"] = st.n_frames_total
            changes["training_batch"] = (st.n_frames_load, st.n_frames_bp)
        if self.fix_global_ends(epoch):
            st.fix_global = False
            changes["update_fixed_params"] = True
        st.epoch, st.epoch_iter = epoch + 1, 0
        return events, changes
