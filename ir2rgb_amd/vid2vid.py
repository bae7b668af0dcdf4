"""The vid2vid inner loop for IR->RGB on MI355X: generator recurrence, reference flow, discriminator
losses, three optimizer steps -- one process per GPU, gradients all-reduced with RCCL.

This is the build's own harness for SURVEY section 8 rows a8, a12, a13, a14 and section 8(e); it
reproduces the semantics of the reference's wrappers without their single-process multi-GPU
placement logic:

    generator recurrence / pyramid      models/generator.py:99-182, :217-235; base_model.py:64-82
    reference flow + confidence         models/flownet.py:20-57
    image / temporal discriminator loss models/discriminator.py:90-200, :236-248, :257-283; models/loss.py:8-41,:105-113
    loop body and optimizer order       train_vid2vid.py:54-111, :166-169

Differences that do not change results: D parameters are frozen during the generator-loss pass
(the reference computes those gradients and discards them with optimizer_d.zero_grad()); the G
gradient all-reduce is overlapped with the D backward; sequences are frame-parallel across ranks.
"""
import contextlib
import os

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import autograd, layers, networks
from . import conv as _conv
from . import streamcheck as SC
from .flatgrads import FlatGrads
from .flownet import FlowNet
from .frames import FrameHistory
from .losses import _SplitGroupsFn, drop_grad_dsts, fused_losses, split_groups  # noqa: F401  (re-exported)
from .networks import SLOT_D_TEMPORAL, SLOT_FLOWNET, _Branch, side_stream
from .optim import (FusedAdam, GradGuard, LossScaler, ParamEMA, check_ema_option, check_grad_guard_option,  # noqa: F401
                    check_loss_scale_option, make_loss_scaler)

DEFAULTS = dict(  # options/base_options.py, options/train_options.py
    input_nc=3, output_nc=3, n_input_gen_frames=3, first_layer_gen_filters=128, gen_network="composite", gen_ds_layers=3,
    gen_blocks=9, n_blocks_local=3, norm="batch", n_scales_spatial=1, fg=False, no_flow=False, n_local_enhancers=1,
    feat_num=3, first_layer_dis_filters=64, num_D=2, n_layers_D=3, no_ganFeat=False, n_frames_D=3, n_scales_temporal=2,
    lr=2e-4, beta1=0.5, lambda_feat=10.0, lambda_T=10.0, lambda_F=10.0, no_first_img=False, max_frames_per_gpu=1,
    n_frames_bp=1, compute_dtype=torch.bfloat16, flownet_dtype=torch.bfloat16,
    no_vgg=True,         # VGG19 perceptual loss off: the pretrained weights cannot be downloaded here (False: ir2rgb_amd.vgg,
                         # randomly initialised unless a torchvision state_dict is loaded into trainer.vgg_loss.vgg)
    shared_fake_forward=True,   # one netD forward on generated frames serves the D and the G loss (autograd.backward_flags)
    resident_inputs=False,      # the window tensors are not written on the main stream (see reference_flows)
    reuse_skipped_flows=True,   # reference flows of temporally skipped frame pairs seen in an earlier window are kept, not recomputed
    allreduce_chunk_elems=32 * 1024 * 1024,   # fp32 elements per gradient all-reduce (128 MB)
    batched_D=True,      # (with shared_fake_forward) real | generated | raw frames go through a discriminator as ONE batch of sample groups
    fused_adam=True,     # one-launch HIP Adam (ir2rgb_amd.optim); False = torch.optim.Adam(foreach=True)
    loss_scale=None,     # f16 training: a number (static scale), "dynamic" (2^16, halved on overflow, doubled after 2000 clean
                         # windows) or an ir2rgb_amd.optim.LossScaler; overflowed windows are skipped on the device.  Needs fused_adam
    max_grad_norm=None,  # guarded optimizer steps for every compute_dtype (ir2rgb_amd.optim.GradGuard): per optimizer a gradient with an inf
                         # or NaN skips the step, a finite one is clipped to this global L2 norm -- decided on the device.  A number for
                         # every optimizer, float("inf") (guard, never clip) or {"G": x, "D": y, "D_T": z} (a missing key: inf).  The
                         # norms come back from train_window as GN_G, GN_D, GN_D_T{s}.  Needs fused_adam.  None: nothing changes
    ema_decay=None,      # a number in [0, 1): trainer.ema (ir2rgb_amd.optim.ParamEMA) averages every generator's parameters after each
                         # generator step, one launch per window; a loss-scaled window that was skipped skips the average too (decided
                         # on the device).  trainer.ema_generators() are the averaged networks for inference.  None: nothing is allocated
    ema_warmup=True,     # the n-th average uses min(ema_decay, (1 + n) / (10 + n)): the first ones follow the parameters closely
    fused_losses=True,   # grouped HIP loss kernels (ir2rgb_amd.losses); False = the same terms through torch ops
    batched_repack=True,  # all packed weight copies refreshed by one launch after the optimizer steps (layers.WeightRepacker)
    build_flow_net=True,  # False: trainer.flow_net is left None for the caller to set (tests plug a stand-in for FlowNet2)
    branch_streams_fine_scales=True,   # the finer spatial scales' generators run their two branches on two HIP streams, forward
                                       # and backward (the coarsest scale's kernels are what bench.py brackets: one stream)
    niter_fix_global=0,  # != 0 with n_scales_spatial > 1: only the finest spatial scale trains until update_fixed_params() (generator.py:64-72)
    TTUR=False,          # two time-scale update rule: G at lr / 2, D at lr * 2, both with betas (0, 0.9) (generator.py:74-79, discriminator.py:77-82)
    lr_policy="reference",   # update_learning_rate: "reference" = what the reference does (G and D get the one decayed value, the temporal
                             # discriminators keep theirs); "all" = every optimizer decays and keeps its TTUR factor
    discriminator_streams=True,        # the image discriminator's scales and the temporal discriminators each on their own HIP stream (forward and, through autograd, backward): independent networks of small layers that fill a fraction of the chip one at a time
)


def avg_pool_pyramid(t, n_scales):
    """[B,T,C,H,W] -> list of n_scales tensors, each AvgPool2d(3,2,1,count_include_pad=False) of the previous
    (base_model.py:64-82)."""
    out = [t]
    for _ in range(1, n_scales):
        b, tt, c, h, w = out[-1].shape
        d = autograd.avg_pool3s2(out[-1].reshape(-1, h, w).unsqueeze(1))
        out.append(d.view(b, tt, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1))
    return out


_GRID_CACHE = {}


def _grid(b, h, w, device, dtype):
    """get_grid once per shape: the lattice is built on the host, so re-creating it costs a synchronous
    host-to-device copy per call (the reference caches it on the module too, base_model.py:131-132)."""
    key = (b, h, w, str(device), dtype)
    if key not in _GRID_CACHE:
        _GRID_CACHE[key] = networks.get_grid(b, h, w, device=device, dtype=dtype)
    return _GRID_CACHE[key]


def resample(image, flow):
    """Model.resample (base_model.py:129-136): same align_corners mismatch as the generator's warp."""
    b, c, h, w = image.shape
    grid = _grid(b, h, w, flow.device, flow.dtype)
    fl = torch.cat([flow[:, 0:1] / ((w - 1.0) / 2.0), flow[:, 1:2] / ((h - 1.0) / 2.0)], 1)
    return F.grid_sample(image, (grid + fl).permute(0, 2, 3, 1), mode="bilinear", padding_mode="border", align_corners=False)


def masked_l1(a, b, mask):
    m = mask.expand(-1, a.size(1), -1, -1)
    return F.l1_loss(a * m, b * m)


def gan_loss(pred, real):
    """GANLoss with gan_mode 'ls' -> MSE against a constant target, summed over the D scales (loss.py:8-41)."""
    total = 0
    for scale in pred:
        p = scale[-1].float()
        total = total + F.mse_loss(p, torch.full_like(p, 1.0 if real else 0.0))
    return total


@contextlib.contextmanager
def frozen(module):
    ps = [p for p in module.parameters() if p.requires_grad]
    for p in ps:
        p.requires_grad_(False)
    try:
        yield
    finally:
        for p in ps:
            p.requires_grad_(True)


class _LossDict(dict):
    """A dict of named loss terms that may also carry them as the vectors the fused loss kernels wrote
    (``vecs`` = (image-term vector | None, discriminator-term vector, generator-term vector), see get_losses)."""
    vecs = None


class Vid2VidTrainer:
    """One rank's models, optimizers and per-sequence state; ``train_window`` is the loop body."""

    def __init__(self, device, world_size=1, seed=0, **overrides):
        o = dict(DEFAULTS)
        o.update(overrides)
        check_loss_scale_option(o["loss_scale"], o["fused_adam"])     # (a ValueError before anything is built)
        check_ema_option(o["ema_decay"])
        self._max_norms = check_grad_guard_option(o["max_grad_norm"], o["fused_adam"])
        if o["lr_policy"] not in ("reference", "all"):
            raise ValueError(f"lr_policy: \"reference\" or \"all\", got {o['lr_policy']!r}")
        self.opt, self.device, self.world = o, device, world_size
        tG = o["n_input_gen_frames"]
        self.n_scales, self.t_scales, self.tD = o["n_scales_spatial"], o["n_scales_temporal"], o["n_frames_D"]
        g_in, g_prev = o["input_nc"] * tG, (tG - 1) * o["output_nc"]
        kw = {k: o[k] for k in ("gen_blocks", "n_local_enhancers", "feat_num", "n_blocks_local", "fg", "no_flow")}
        torch.manual_seed(seed)  # identical initial weights on every rank
        self.netG = [networks.build_generator_module(g_in, o["output_nc"], g_prev, o["first_layer_gen_filters"],
                                                      o["gen_network"], o["gen_ds_layers"], o["norm"], 0, **kw)]
        for s in range(1, self.n_scales):
            self.netG.append(networks.build_generator_module(g_in, o["output_nc"], g_prev, o["first_layer_gen_filters"] // 2 ** s,
                                                             o["gen_network"] + "-local", o["gen_ds_layers"], o["norm"], s, **kw))
        self.netD = networks.build_discriminator_module(o["input_nc"] + o["output_nc"], o["first_layer_dis_filters"],
                                                        o["n_layers_D"], o["norm"], o["num_D"], not o["no_ganFeat"])
        dt_in = o["output_nc"] * self.tD + 2 * (self.tD - 1)
        self.netD_T = [networks.build_discriminator_module(dt_in, o["first_layer_dis_filters"], o["n_layers_D"], o["norm"],
                                                           o["num_D"], not o["no_ganFeat"]) for _ in range(self.t_scales)]
        for m in self.netG + [self.netD] + self.netD_T:
            m.to(device).train()
            m.compute_dtype = o["compute_dtype"]
        # ---- the schedule: every stream decision and every environment variable the trainer honours, read once
        cuda = device.type == "cuda"
        # gloo (the CPU-side rehearsal backend of bench.py) moves CUDA tensors through the host and synchronises the device:
        # next to it a second stream is pathological (two-rank rehearsal: 7.9 s per window with the finer-scale generators'
        # branches on two streams, 0.39 s without; 7.6 s with FlowNet2's replay on a second stream, 0.43 s on the main one;
        # the discriminators' streams cost 30 ms there).  RCCL ranks keep all streams (tests/test_rccl_gpu.py: bit-identical
        # to the single-process trainer next to RCCL's collectives).
        gloo = world_size > 1 and not (dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl")
        for g in self.netG[1:]:
            g.branch_streams_training = bool(o["branch_streams_fine_scales"]) and not gloo
        self.d_streams = bool(o["discriminator_streams"]) and cuda
        self.netD.scale_streams = self.d_streams
        # FlowNet2 is replayed from a HIP graph in every configuration (a capture next to a process group runs in
        # thread-local mode, FlowNet.compute_flow_and_conf), on its own stream unless IR2RGB_FLOW_STREAM=0 (or gloo)
        self.flow_stream_on = cuda and not gloo and os.environ.get("IR2RGB_FLOW_STREAM", "1") != "0"
        self.flow_net = None
        if o["build_flow_net"]:
            self.flow_net = FlowNet(o["flownet_dtype"], use_graph=None).to(device)
        self._side_wgrad = None          # set per window in generate(): safe only when n_load == 1
        self.schedule = self._batch_state = None    # attach_schedule()
        self.old_lr = o["lr"]            # the rate without any TTUR factor (base_model.py:98-99, :105)
        self.last_outputs = None         # (fake_B, fake_B_raw, flow, weight) of the last train_window
        self.last_inputs = None          # (real_A, real_B, flow_ref, conf_ref) of the last train_window
        self.vgg_loss = None
        if not o["no_vgg"]:
            from .vgg import VGGLoss
            self.vgg_loss = VGGLoss().to(device)
            self.vgg_loss.vgg.compute_dtype = o["compute_dtype"]

        # finest-scale-only epochs (generator.py:64-72): the coarser generators get no gradient buffer and no moments
        self.finetune_all = o["niter_fix_global"] == 0 or self.n_scales == 1
        # TTUR (generator.py:74-79, discriminator.py:77-82); the temporal discriminators keep lr and (beta1, 0.999)
        plain = (1.0, (o["beta1"], 0.999))
        self._rule_G, self._rule_D = ((0.5, (0.0, 0.9)), (2.0, (0.0, 0.9))) if o["TTUR"] else (plain, plain)
        self._rule_DT = plain
        self.grads_G = self._make_grads_G()
        self.grads_D = FlatGrads(self.netD.parameters())
        self.grads_DT = [FlatGrads(d.parameters()) for d in self.netD_T]
        self.optimizer_G = self._make_optimizer(self.grads_G.params, o["lr"] * self._rule_G[0], self._rule_G[1])
        self.optimizer_D = self._make_optimizer(self.grads_D.params, o["lr"] * self._rule_D[0], self._rule_D[1])
        self.optimizer_D_T = [self._make_optimizer(g.params, o["lr"], self._rule_DT[1]) for g in self.grads_DT]
        self.loss_scaler = make_loss_scaler(o["loss_scale"], device)
        self._register_scaler_tables()
        # one guard per optimizer (max_grad_norm), in the order of its family; a replaced guard's counters are carried here
        self.grad_guards = self._stepped = None
        self._guard_carry = {"steps": 0, "clipped": 0, "skipped": 0}
        if self._max_norms is not None:
            self.grad_guards = {"G": GradGuard(self.optimizer_G, self._max_norms["G"]),
                                "D": GradGuard(self.optimizer_D, self._max_norms["D"]),
                                "D_T": [GradGuard(o_, self._max_norms["D_T"]) for o_ in self.optimizer_D_T]}
        # the average of ALL generators' parameters, whatever niter_fix_global says: a fixed scale's average equals its
        # parameters (p == e leaves e as it is) until update_fixed_params(), which leaves the average alone
        self.ema = self._ema_netG = None
        if o["ema_decay"] is not None:
            self.ema = ParamEMA([p for g in self.netG for p in g.parameters()], o["ema_decay"], o["ema_warmup"])
        self.repacker = layers.WeightRepacker(list(self.netG) + [self.netD] + list(self.netD_T)) if o["batched_repack"] else None
        self.reset_sequence()

    def _make_grads_G(self):
        """The generator optimizer's gradient buffer: every scale, or the finest one alone while the coarser ones are fixed."""
        o = self.opt
        nets = self.netG if self.finetune_all else self.netG[-1:]
        g_params = [p for g in nets for p in g.parameters()]
        # (generators: one use per parameter and pass when one frame is generated per window, see generate())
        return FlatGrads(g_params, chunk_elems=o["allreduce_chunk_elems"], world=self.world, direct=o["max_frames_per_gpu"] == 1)

    def _make_optimizer(self, params, lr, betas):
        if self.opt["fused_adam"]:
            return FusedAdam(params, lr=lr, betas=betas)
        # NOT fused=True: torch's fused Adam updates the parameters without bumping their version counters,
        # and the packed MFMA weights (ir2rgb_amd.layers.packed_weight) are refreshed on a version change
        return torch.optim.Adam(params, lr=lr, betas=betas, foreach=True)

    def _register_scaler_tables(self):
        if self.loss_scaler is not None:        # the device tables of every window's optimizer set, ahead of the loop
            for n in range(self.t_scales + 1):
                self.loss_scaler.register([self.optimizer_G, self.optimizer_D] + self.optimizer_D_T[:n])

    # ------------------------------------------------------------------ between epochs (ir2rgb_amd.schedule, ir2rgb_amd.training)
    def update_fixed_params(self):
        """Model.update_fixed_params (base_model.py:101-107): from here on every scale trains.  A new ``optimizer_G`` over
        all scales with fresh moments and step count 0, as the reference builds it: at ``old_lr`` -- the initial rate or the
        last decayed one -- with betas (beta1, 0.999), i.e. without TTUR's factor and betas.  ``lr_policy="all"`` keeps both.
        The gradient buffer, the side-stream / in-place weight-gradient arrangement and the loss scaler's device tables
        are rebuilt to match."""
        if self.finetune_all:
            return
        o = self.opt
        keep = o["lr_policy"] == "all"
        lr = self.old_lr * (self._rule_G[0] if keep else 1.0)
        betas = self._rule_G[1] if keep else (o["beta1"], 0.999)
        self.grads_G.close()
        self.finetune_all = True
        self.grads_G = self._make_grads_G()
        self.optimizer_G = self._make_optimizer(self.grads_G.params, lr, betas)
        self._side_wgrad = None                 # generate() re-runs enable_side_wgrad / set_direct for the next window
        if self.loss_scaler is not None:
            self.loss_scaler.forget_tables()
            self._register_scaler_tables()
        if self.grad_guards is not None:        # (reads the old guard's counters: synchronises, between epochs)
            old = self.grad_guards["G"].stats()
            for k in self._guard_carry:
                self._guard_carry[k] += old[k]
            self.grad_guards["G"] = GradGuard(self.optimizer_G, self._max_norms["G"])
            self._stepped = None

    def grad_guard_stats(self):
        """{"G": {...}, "D": {...}, "D_T": [{...}, ...]}: every guard's ``GradGuard.stats()`` (``max_grad_norm``), the
        generator's counters including those of the guard ``update_fixed_params`` replaced.  Synchronises."""
        if self.grad_guards is None:
            raise ValueError("grad_guard_stats: the trainer was built without max_grad_norm")
        g = self.grad_guards["G"].stats()
        for k, v in self._guard_carry.items():
            g[k] += v
        return {"G": g, "D": self.grad_guards["D"].stats(), "D_T": [x.stats() for x in self.grad_guards["D_T"]]}

    def decided_optimizers(self):
        """The optimizers stepped in the last window when their steps were guarded (what ``LossLog.push`` asks whether
        the window was skipped); None without ``max_grad_norm``: the log then asks the loss scaler, if there is one."""
        return self._stepped

    def ema_generators(self):
        """The averaged generators (``ema_decay``): modules built once with the trainer's options whose parameters ARE the
        views of ``trainer.ema``'s shadow buffer (``requires_grad=False``; nothing is copied per window, and their packed
        half weights refresh on their next forward because every update moves the version counters).  BatchNorm running
        statistics and ``num_batches_tracked`` are not averaged: they are copied from the live generators at each call."""
        if self.ema is None:
            raise ValueError("ema_generators: the trainer was built without ema_decay")
        if self._ema_netG is None:
            from .inference import VideoTranslator
            with torch.random.fork_rng(devices=[]):         # (the modules' initialisation draws: not from the trainer's stream)
                gens = VideoTranslator._build_generators(self.opt)
            i = 0
            for g in gens:
                for name, p in list(g.named_parameters()):
                    owner, _, leaf = name.rpartition(".")
                    view = self.ema.shadow(i)
                    assert view.shape == p.shape, name
                    (g.get_submodule(owner) if owner else g)._parameters[leaf] = torch.nn.Parameter(view, requires_grad=False)
                    i += 1
                g.to(self.device).train()                   # (moves the buffers; the parameters are on the device already)
                g.compute_dtype = self.opt["compute_dtype"]
            assert i == len(self.ema.params)
            self._ema_netG = gens
        layers.flush_bn_counters()
        with torch.no_grad():
            for g, live in zip(self._ema_netG, self.netG):
                for b, src in zip(g.buffers(), live.buffers()):
                    b.copy_(src)
        return self._ema_netG

    def attach_schedule(self, schedule):
        """The ``ir2rgb_amd.schedule.TrainingSchedule`` whose arithmetic ``update_learning_rate`` and ``update_training_batch``
        apply (``ir2rgb_amd.training.fit`` attaches its own).  Its ``lr`` has to be the trainer's."""
        if schedule.lr != self.opt["lr"]:
            raise ValueError(f"schedule.lr {schedule.lr!r} differs from the trainer's lr {self.opt['lr']!r}")
        self.schedule = schedule
        self._batch_state = schedule.initial_training_batch()

    def update_learning_rate(self, epoch):
        """Model.update_learning_rate (base_model.py:94-99) as models.py:112-116 calls it for G and D: the schedule's
        ``lr_after(epoch)`` assigned to ``param_groups[...]["lr"]``, which the optimizers read per step.
        ``lr_policy="reference"``: exactly that -- optimizer_G and optimizer_D get the one value (a TTUR factor is gone from
        then on) and the temporal discriminators' optimizers are never touched.  ``lr_policy="all"``: every optimizer gets
        the value times its own factor.  -> the decayed value."""
        lr = self.old_lr = self.schedule.lr_after(epoch)
        if self.opt["lr_policy"] == "reference":
            targets = [(self.optimizer_G, 1.0), (self.optimizer_D, 1.0)]
        else:
            targets = [(self.optimizer_G, self._rule_G[0]), (self.optimizer_D, self._rule_D[0])] + \
                      [(d, self._rule_DT[0]) for d in self.optimizer_D_T]
        for opt, factor in targets:
            for group in opt.param_groups:
                group["lr"] = lr * factor
        return lr

    def update_training_batch(self, ratio, resume=False):
        """Model.update_training_batch (base_model.py:109-120), the arithmetic being the schedule's: the number of frames
        the loss is backpropagated through becomes ``opt["n_frames_bp"]``; -> ``n_frames_load``, the frames per window the
        slicer is to cut (``generate`` reads it off the window it is given).  ``resume``: the state an uninterrupted run
        holds after the call for ``ratio``, from the initial one."""
        if resume:
            self._batch_state = self.schedule.initial_training_batch()
            for r in range(1, ratio + 1):
                self._batch_state = self.schedule.update_training_batch(*self._batch_state, r)
        else:
            self._batch_state = self.schedule.update_training_batch(*self._batch_state, ratio)
        self.opt["n_frames_bp"] = self._batch_state[1]
        return self._batch_state[0]

    def _flow_stream(self, t):
        """The side stream FlowNet2 runs on (None: same stream as everything else)."""
        if not self.flow_stream_on or not t.is_cuda or not isinstance(self.flow_net, FlowNet):
            return None
        return side_stream(t.device, SLOT_FLOWNET)

    # ------------------------------------------------------------------ per-sequence state
    def reset_sequence(self):
        self.fake_B_prev = None          # pyramid of the last tG-1 generated frames
        self._pair_flows = {}            # temporal scale -> [(push count, flow, conf)] of its newest pairs (reference_flows)
        self._early_on = False           # FlowNet2 ahead of the main stream (reference_flows)
        self._backward_done = None       # event: the previous window's backward passes are through
        # histories of the four streams the temporal discriminators sub-sample (train_vid2vid.py:45-52: real_B_all,
        # fake_B_all, flow_ref_all, conf_ref_all), each in one preallocated device buffer (ir2rgb_amd.frames)
        ts, tD = self.t_scales, self.tD
        self.hist = {"real": FrameHistory(ts, tD), "fake": FrameHistory(ts, tD), "flow": FrameHistory(1, tD),
                     "conf": FrameHistory(1, tD)}

    # ------------------------------------------------------------------ generator (a8)
    def generate(self, real_A_all, real_B_all):
        """One window: [B, n_frames_load + tG - 1, C, H, W] inputs -> the reference's 7-tuple
        (generator.py:99-123)."""
        tG, ns = self.opt["n_input_gen_frames"], self.n_scales
        n_load = real_A_all.size(1) - tG + 1
        if self._side_wgrad != (n_load == 1):
            # every generator is applied once per backward pass when one frame is generated per window:
            # only then may its weight gradients run on the side stream (ir2rgb_amd.autograd) ...
            self._side_wgrad = n_load == 1
            for g in self.netG:
                autograd.enable_side_wgrad(g, self._side_wgrad)
        # ... and only then may they be written straight into the all-reduce buffer (FlatGrads.set_direct)
        self.grads_G.set_direct(n_load == 1)
        first = self.fake_B_prev is None
        if not first:
            fake_pyr = list(self.fake_B_prev)
        elif self.opt["no_first_img"]:       # the model also generates the first frame (generator.py:219-220)
            fake_pyr = avg_pool_pyramid(torch.zeros_like(real_B_all[:, :tG - 1]), ns)
        else:                                # training: the first frames are given (generator.py:221-222)
            fake_pyr = avg_pool_pyramid(real_B_all[:, :tG - 1], ns)
        A_pyr = avg_pool_pyramid(real_A_all, ns)
        fake_raw, flows, weights = [], [], []
        for t in range(n_load):
            feat = flow_feat = None
            for s in range(ns):                      # coarse to fine
                si = ns - 1 - s
                As = A_pyr[si]
                b, _, _, h, w = As.shape
                A_in = As[:, t:t + tG].reshape(b, -1, h, w)
                prev = fake_pyr[si][:, t:t + tG - 1]
                if t % self.opt["n_frames_bp"] == 0:
                    prev = prev.detach()
                # finest-scale-only epochs: the coarser scales' results enter the next scale detached (generator.py:166-172).
                # They run in training mode (their BatchNorm running statistics advance) but without a tape: same kernels,
                # same bits, no saved activations and no backward pass
                fixed = s != ns - 1 and not self.finetune_all
                with (torch.no_grad() if fixed else contextlib.nullcontext()):
                    out = self.netG[s](A_in, prev.reshape(b, -1, h, w), None, feat, flow_feat, None,
                                       self.opt["no_first_img"] and first)
                fake_B, flow, weight, raw, feat, flow_feat, _ = out
                fake_pyr[si] = torch.cat([fake_pyr[si], fake_B.unsqueeze(1)], 1)
                if s == ns - 1:
                    fake_raw.append(raw.unsqueeze(1))
                    flows.append(flow.unsqueeze(1))
                    weights.append(weight.unsqueeze(1))
        self.fake_B_prev = [B[:, -tG + 1:].detach() for B in fake_pyr]
        fake_B = fake_pyr[0][:, tG - 1:]
        one = lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts, 1)  # noqa: E731  (one frame per window: no copy)
        return (fake_B, one(fake_raw), one(flows), one(weights), real_A_all[:, tG - 1:], real_B_all[:, tG - 2:])

    # ------------------------------------------------------------------ discriminator losses (a13)
    def _gan_and_fm(self, pred_real, pred_fake):
        o = self.opt
        fw, dw = 4.0 / (o["n_layers_D"] + 1), 1.0 / o["num_D"]
        if o["fused_losses"]:
            return self._fused_D_terms(pred_real, [pred_fake])[1].unbind(0)
        loss_gan = gan_loss(pred_fake, True)
        loss_fm = torch.zeros_like(loss_gan)
        if not o["no_ganFeat"]:
            for i in range(min(len(pred_fake), o["num_D"])):
                for j in range(len(pred_fake[i]) - 1):
                    loss_fm = loss_fm + dw * fw * (pred_fake[i][j] - pred_real[i][j].detach()).abs().mean(dtype=torch.float32) * o["lambda_feat"]
        return loss_gan, loss_fm

    def _fused_D_terms(self, pred_real, pred_fakes):
        """compute_loss_D (discriminator.py:154-166, :186-200) for every generated input in ``pred_fakes`` against the same
        real forward, as TWO loss launches: the discriminator-side vector [D_real, D_fake] and the generator-side vector
        [G_GAN, G_GAN_Feat], each already summed over the inputs.  (Two groups, not one: a backward pass then differentiates
        only the group its total depends on, and every prediction tensor receives one gradient per pass.)  The real
        logits appear in one term of weight len(pred_fakes): the reference evaluates that term once per compute_loss_D call
        on identical activations -- two terms on one tensor would write one gradient destination twice (losses._take_dst)."""
        o = self.opt
        fw, dw = 4.0 / (o["n_layers_D"] + 1), 1.0 / o["num_D"]
        k = float(len(pred_fakes))
        d_terms = [("mse", scale[-1], 1.0, k, 0) for scale in pred_real]
        g_terms = []
        for pf in pred_fakes:
            d_terms += [("mse", scale[-1], 0.0, 1.0, 1) for scale in pf]
            g_terms += [("mse", scale[-1], 1.0, 1.0, 0) for scale in pf]
            if not o["no_ganFeat"]:
                for i in range(min(len(pf), o["num_D"])):
                    for j in range(len(pf[i]) - 1):
                        g_terms.append(("l1", pf[i][j], pred_real[i][j], dw * fw * o["lambda_feat"], 1))
        return fused_losses(d_terms, 2, o["compute_dtype"]), fused_losses(g_terms, 2, o["compute_dtype"])

    def _loss_D(self, netD, real_in, fake_in, pred_real=None, pred_fake=None):
        """Three forwards exactly as compute_loss_D (discriminator.py:154-166).  ``pred_real`` / ``pred_fake``: the results
        of ``netD(real_in)`` / ``netD(fake_in)`` when the caller already holds them (see image_losses, _batched_D)."""
        if pred_real is None:
            pred_real = netD(real_in)
        shared = self.opt["shared_fake_forward"]
        if pred_fake is not None:
            pred_fake_d = pred_fake
        elif shared:
            with layers.repeated_forward(2):
                pred_fake_d = pred_fake = netD(fake_in)
        else:
            pred_fake_d = netD(fake_in.detach())
        if self.opt["fused_losses"] and pred_fake is not None:
            dvec, gvec = self._fused_D_terms(pred_real, [pred_fake])
            return tuple(dvec.unbind(0)) + tuple(gvec.unbind(0))
        if self.opt["fused_losses"]:
            out = fused_losses([("mse", scale[-1], 1.0, 1.0, 0) for scale in pred_real] +
                               [("mse", scale[-1], 0.0, 1.0, 1) for scale in pred_fake_d], 2, self.opt["compute_dtype"])
            loss_D_real, loss_D_fake = out[0], out[1]
        else:
            loss_D_real, loss_D_fake = gan_loss(pred_real, True), gan_loss(pred_fake_d, False)
        if pred_fake is None:
            with frozen(netD):
                pred_fake = netD(fake_in)
        loss_G_GAN, loss_G_FM = self._gan_and_fm(pred_real, pred_fake)
        return loss_D_real, loss_D_fake, loss_G_GAN, loss_G_FM

    def _batched_D(self, netD, inputs, repeats, order=None):
        """``netD`` on several inputs as ONE batch of sample groups (MultiScaleDiscriminator.forward): every convolution
        and every weight gradient runs once per layer instead of once per input, BatchNorm sees each input as the
        separate forward it is in the reference (``repeats[g]``: how many reference forwards group g stands for, i.e.
        how often its batch statistics enter the running statistics; ``order``: the order the groups' statistics enter
        them in).  Callers put the generated frames FIRST: the generator's backward pass then works on the leading
        groups only (autograd.backward_flags(active_groups=...)).  -> one prediction pyramid per input."""
        G = len(inputs)
        owner = next(m for m in netD.modules() if isinstance(m, torch.nn.Conv2d))
        # gradient destinations registered by this network's previous forward are dropped here: an entry lives from one
        # forward of a network to its next, whoever the caller is (the registry is keyed by address)
        drop_grad_dsts(owner)
        with layers.repeated_forward(tuple(repeats)):
            out = netD(torch.cat(inputs, 0), sample_groups=G, group_order=order)
        preds = [[[] for _ in out] for _ in range(G)]
        for i, scale in enumerate(out):
            for t in scale:
                for g, piece in enumerate(split_groups(t, G, owner)):
                    preds[g][i].append(piece)
        return preds

    def image_losses(self, real_B, fake_B, fake_B_raw, real_A, real_B_prev, fake_B_prev, flow, weight, flow_ref, conf_ref):
        o = self.opt
        L = _LossDict()
        wF, wT = o["lambda_F"] / (2 ** (self.n_scales - 1)), o["lambda_T"]
        imgvec = None
        if o["fused_losses"]:
            terms = [("ml1", flow, flow_ref, conf_ref, wF, 0),
                     ("ml1", resample(real_B_prev, flow), real_B, conf_ref, wT, 1),
                     ("ml1", fake_B, resample(fake_B_prev, flow_ref), conf_ref, wT, 3)]
            if o["no_first_img"]:
                terms.append(("ml1", weight, None, conf_ref, 1.0, 2))
            imgvec = fused_losses(terms, 4, o["compute_dtype"])
            L["F_Flow"], L["F_Warp"], L["W"], L["G_Warp"] = imgvec.unbind(0)
        else:
            L["F_Flow"] = masked_l1(flow, flow_ref, conf_ref) * wF
            L["F_Warp"] = masked_l1(resample(real_B_prev, flow), real_B, conf_ref) * wT
            L["W"] = masked_l1(weight, torch.zeros_like(weight), conf_ref) if o["no_first_img"] else torch.zeros((), device=flow.device)
            L["G_Warp"] = masked_l1(fake_B, resample(fake_B_prev, flow_ref).detach(), conf_ref) * wT
        if o["no_vgg"]:
            L["G_VGG"] = torch.zeros((), device=flow.device)  # VGG19 weights are not available offline (no_vgg)
        else:   # discriminator.py:132-133, :141-142
            L["G_VGG"] = (self.vgg_loss(fake_B, real_B) + self.vgg_loss(fake_B_raw, real_B)) * o["lambda_feat"]
        # The reference calls compute_loss_D twice (final and raw image, discriminator.py:125-131) and each call
        # evaluates netD on the same real pair with the same weights: identical activations, so it is
        # evaluated once here and counted twice (BatchNorm running statistics advance twice as well;
        # reference call sites discriminator.py:134 and :143).
        real_in = torch.cat((real_A, real_B), 1)
        fake_in, raw_in = torch.cat((real_A, fake_B), 1), torch.cat((real_A, fake_B_raw), 1)
        if o["batched_D"] and o["shared_fake_forward"]:
            pred_fake, pred_raw, pred_real = self._batched_D(self.netD, [fake_in, raw_in, real_in], (2, 2, 2), (2, 0, 1))
        else:
            with layers.repeated_forward(2):
                pred_real = self.netD(real_in)
            pred_fake = pred_raw = None
        if o["fused_losses"] and pred_fake is not None:
            # both compute_loss_D calls in two launches; the sums D_real + D_real2 ... are formed inside the kernels
            dvec, gvec = self._fused_D_terms(pred_real, [pred_fake, pred_raw])
            L["D_real"], L["D_fake"] = dvec.unbind(0)
            L["G_GAN"], L["G_GAN_Feat"] = gvec.unbind(0)
            L.vecs = (imgvec, dvec, gvec)
            return L
        d_real, d_fake, g_gan, g_fm = self._loss_D(self.netD, real_in, fake_in, pred_real, pred_fake)
        d_real2, d_fake2, g_gan2, g_fm2 = self._loss_D(self.netD, real_in, raw_in, pred_real, pred_raw)
        L["D_real"], L["D_fake"] = d_real + d_real2, d_fake + d_fake2
        L["G_GAN"], L["G_GAN_Feat"] = g_gan + g_gan2, g_fm + g_fm2
        return L

    def temporal_losses(self, s, real_B, fake_B, flow_ref, conf_ref):
        """compute_loss_D_T (discriminator.py:168-184) for temporal scale s."""
        b = real_B.size(0)
        h, w = real_B.shape[-2:]
        fl = (flow_ref / 20).reshape(b, -1, h, w)
        real_in = torch.cat([real_B.reshape(b, -1, h, w), fl], 1)
        fake_in = torch.cat([fake_B.reshape(b, -1, h, w), fl], 1)
        if self.opt["batched_D"] and self.opt["shared_fake_forward"]:
            pred_fake, pred_real = self._batched_D(self.netD_T[s], [fake_in, real_in], (2, 1), (1, 0))
            if self.opt["fused_losses"]:
                dvec, gvec = self._fused_D_terms(pred_real, [pred_fake])
                LT = _LossDict(zip(("D_T_real", "D_T_fake", "G_T_GAN", "G_T_GAN_Feat"), tuple(dvec.unbind(0)) + tuple(gvec.unbind(0))))
                LT.vecs = (None, dvec, gvec)
                return LT
            d_real, d_fake, g_gan, g_fm = self._loss_D(self.netD_T[s], real_in, fake_in, pred_real, pred_fake)
        else:
            d_real, d_fake, g_gan, g_fm = self._loss_D(self.netD_T[s], real_in, fake_in)
        return {"D_T_real": d_real, "D_T_fake": d_fake, "G_T_GAN": g_gan, "G_T_GAN_Feat": g_fm}

    # ------------------------------------------------------------------ temporal frame bookkeeping
    # get_skipped_frames (discriminator.py:257-271) lives in ir2rgb_amd.frames.FrameHistory.push: one preallocated
    # device buffer per stream instead of a torch.cat of the whole history per window.
    def reference_flows(self, real_B, real_B_prev, side=None):
        """All FlowNet2 evaluations of one window in ONE batched call: the reference flow of the current
        frame (train_vid2vid.py:65) and the flows of the temporally skipped real triplets
        (discriminator.py:281-283).  Both depend on real frames only, so batching them changes nothing
        numerically (FlowNet2 is per-sample, frozen, eval mode)."""
        ts = self.t_scales
        # ``resident_inputs`` (the window tensors are not produced on the main stream: bench.py's synthetic sequence, a
        # loader that prefetches on its own stream and has synchronised): the real-frame bookkeeping and FlowNet2's replay
        # then run on the second stream WITHOUT waiting for the main stream, i.e. beside the previous window's optimizer
        # step (2.7 ms of pure HBM streaming) as well as beside this window's generator forward.  Only for replays.
        early = False
        if side is not None and self.opt["resident_inputs"] and isinstance(self.flow_net, FlowNet) and real_B.shape[1] == 1:
            early = self.flow_net.will_replay(self._count_pairs(real_B), real_B.reshape((-1,) + tuple(real_B.shape[2:])))
        main = torch.cuda.current_stream(real_B.device) if real_B.is_cuda else None
        if early:
            if not self._early_on:                          # first time: the histories were last written on the main stream
                side.wait_stream(main)
                self._early_on = True
            if self._backward_done is not None:
                # not before the previous window's generator backward pass is through: the host runs windows ahead of the
                # GPU, and a FlowNet2 that started whenever it was issued would also share the chip with that pass's
                # compute-bound convolutions (no gain, and it spoils bench.py's per-kernel brackets); beside the
                # discriminators' latency-bound passes and the HBM-bound optimizer step it is what fills the chip
                side.wait_event(self._backward_done)
            with torch.cuda.stream(side):
                return self._reference_flows(real_B, real_B_prev, side)
        if self._early_on:                                  # back to the main stream (a new shape: lazy work ahead)
            main.wait_stream(side)
            self._early_on = False
        return self._reference_flows(real_B, real_B_prev, side)

    def _count_pairs(self, real_B):
        """Frame pairs FlowNet2 will see for this one-frame push (host arithmetic only: what _reference_flows is about to
        assemble -- the frame itself, plus per temporal scale whose tuple exists the newest pair, or all tD-1 of them)."""
        h, b = self.hist["real"], real_B.shape[0]
        total, pushed = h.len + 1, h.pushed + 1
        reuse = self.opt["reuse_skipped_flows"] and self.tD == 3
        n = b
        for s in range(1, self.t_scales):
            step = self.tD ** s
            if total - step * (self.tD - 1) >= 1:
                hit = reuse and any(e[0] == pushed - step for e in self._pair_flows.get(s, []))
                n += b * (1 if hit else self.tD - 1)
        return n

    def _reference_flows(self, real_B, real_B_prev, side):
        ts = self.t_scales
        rb_s = self.hist["real"].push(real_B)
        pushed = self.hist["real"].pushed
        firsts, seconds, owners = [real_B.reshape((-1,) + tuple(real_B.shape[2:]))], [real_B_prev.reshape((-1,) + tuple(real_B.shape[2:]))], []
        # Of the tD-1 frame pairs of a temporally skipped tuple (frames tD**s apart) only the newest is new: with one frame
        # per window, pair k of this window is pair k+1 of the window tD**s pushes ago (same two real frames; FlowNet2 is
        # frozen and per-sample), so its flow and confidence are kept instead of being recomputed (the reference recomputes
        # them, discriminator.py:281-283; a third of its FlowNet2 work per window at t_scales 2 / tD 3).
        reuse = self.opt["reuse_skipped_flows"] and real_B.shape[1] == 1 and self.tD == 3     # (tD 3: one older pair per tuple)
        cached = {}
        for s in range(1, ts):
            if rb_s[s] is not None and rb_s[s].size(1) == self.tD:
                a, b = rb_s[s][:, 1:], rb_s[s][:, :-1]
                old = self._pair_flows.get(s, [])
                hit = [e for e in old if e[0] == pushed - self.tD ** s] if reuse else []
                if hit:
                    cached[s] = hit[0]
                    a, b = a[:, -1:], b[:, -1:]                          # only the newest pair goes through FlowNet2
                firsts.append(a.reshape((-1,) + tuple(a.shape[2:])))
                seconds.append(b.reshape((-1,) + tuple(b.shape[2:])))
                owners.append((s, a.shape[0], a.shape[1]))
        if side is not None and isinstance(self.flow_net, FlowNet):
            flow, conf = self.flow_net(torch.cat(firsts), torch.cat(seconds), side=side)
        else:
            flow, conf = self.flow_net(torch.cat(firsts), torch.cat(seconds))
        n0 = firsts[0].shape[0]
        b, t = real_B.shape[:2]
        h, w = real_B.shape[-2:]
        flow_ref, conf_ref = flow[:n0].view(b, t, 2, h, w), conf[:n0].view(b, t, 1, h, w)
        extra, off = {}, n0
        # FlowNet2 may have replayed on the second stream, which the main stream joins only before the losses
        # (train_window): the concatenation below reads its result, so it has to be queued on that stream too
        ran = getattr(self.flow_net, "ran_on", None) if isinstance(self.flow_net, FlowNet) else None
        on_side = ran is not None and torch.cuda.current_stream(flow.device) != ran
        with (torch.cuda.stream(ran) if on_side else contextlib.nullcontext()):
            extra = self._assemble_pair_flows(flow, conf, owners, cached, n0, pushed, reuse, h, w)
        return flow_ref, conf_ref, rb_s, extra

    def _assemble_pair_flows(self, flow, conf, owners, cached, off, pushed, reuse, h, w):
        extra = {}
        for s, bb, tt in owners:
            fl, cf = flow[off:off + bb * tt].view(bb, tt, 2, h, w), conf[off:off + bb * tt].view(bb, tt, 1, h, w)
            off += bb * tt
            if reuse:       # the newest pair's result serves the windows to come (tD - 2 more uses, tD**s pushes apart)
                keep = [e for e in self._pair_flows.get(s, []) if e[0] > pushed - self.tD ** s * (self.tD - 2)]
                self._pair_flows[s] = keep + [(pushed, fl[:, -1:], cf[:, -1:])]
                if SC.ENABLED:
                    SC.consumed(flow, "reference flow (FlowNet2 replay)")
                    SC.produced(fl[:, -1:], "kept pair flow"), SC.produced(cf[:, -1:], "kept pair confidence")
            if s in cached:                                              # (tD == 3: exactly one older pair)
                if fl.is_cuda:
                    for t in cached[s][1:]:
                        t.record_stream(torch.cuda.current_stream(fl.device))   # (it may have been made on the other stream)
                if SC.ENABLED:
                    SC.consumed(flow, "reference flow (FlowNet2 replay)")
                    SC.consumed(cached[s][1], "kept pair flow"), SC.consumed(cached[s][2], "kept pair confidence")
                fl, cf = torch.cat([cached[s][1], fl], 1), torch.cat([cached[s][2], cf], 1)
            extra[s] = (fl, cf)
        return extra

    def skipped_frames(self, rb_s, extra_flows, fake_B, flow_ref, conf_ref):
        """get_all_skipped_frames, dense variant (discriminator.py:219-234, :273-283); the real-frame
        bookkeeping and the FlowNet2 calls were done by reference_flows."""
        ts = self.t_scales
        fb_s = self.hist["fake"].push(fake_B)
        fl0, cf0 = self.hist["flow"].push(flow_ref), self.hist["conf"].push(conf_ref)
        fl_s, cf_s = [None] * ts, [None] * ts
        if fl0[0] is not None:
            fl_s[0], cf_s[0] = fl0[0][:, 1:], cf0[0][:, 1:]
        for s in range(1, ts):
            if s in extra_flows:
                fl_s[s], cf_s[s] = extra_flows[s]
        return rb_s, fb_s, fl_s, cf_s

    # ------------------------------------------------------------------ the loop body (a14)
    def get_losses(self, L, LT):
        """Vid2VidModelD.get_losses (discriminator.py:236-248): ``L`` the image-loss dict, ``LT`` the list of temporal
        dicts of the active temporal scales.  Returns (loss_G, loss_D, [loss_D_T per active scale]).
        Dicts that came out of the fused loss kernels carry their terms as vectors (``_LossDict.vecs``):
        the totals are then one concatenation + one sum for loss_G and one sum per discriminator -- not ~45 scalar adds
        forward and as many select / add nodes backward."""
        mine = [getattr(d, "vecs", None) for d in [L] + list(LT)]
        if all(v is not None for v in mine) and mine[0][0] is not None:
            imgvec, dvec, gvec = mine[0]
            g_parts = [imgvec, gvec] + [m[2] for m in mine[1:]]
            loss_G = torch.cat(g_parts).sum()
            if not self.opt["no_vgg"]:
                loss_G = loss_G + L["G_VGG"]
            loss_D = dvec.sum() * 0.5
            return loss_G, loss_D, [m[1].sum() * 0.5 for m in mine[1:]]
        loss_D = (L["D_fake"] + L["D_real"]) * 0.5
        loss_G = L["G_GAN"] + L["G_GAN_Feat"] + L["G_VGG"] + L["G_Warp"] + L["F_Flow"] + L["F_Warp"] + L["W"]
        loss_D_T = []
        for lt in LT:                                            # G_T_Warp is identically zero (discriminator.py:106)
            loss_G = loss_G + lt["G_T_GAN"] + lt["G_T_GAN_Feat"]
            loss_D_T.append((lt["D_T_fake"] + lt["D_T_real"]) * 0.5)
        return loss_G, loss_D, loss_D_T

    def backward_passes(self, loss_G, loss_D, loss_D_T, g_inputs=None):
        """The three ``loss.backward()`` of train_vid2vid.py:104-111 (zero_grad included); each optimizer's gradient
        all-reduce is issued as soon as its pass ends, so it overlaps the next pass.  ``g_inputs``: the tensors
        the generator's pass differentiates with respect to (default: the generator parameters)."""
        self.grads_G.zero()
        self.grads_D.zero()
        for gdt in self.grads_DT:
            gdt.zero()
        shared = self.opt["shared_fake_forward"]
        d_nets = [self.netD] + self.netD_T
        if g_inputs is None and shared:
            g_inputs = self.grads_G.params
        # shared discriminator forwards are walked twice: by the generator's pass (frames only) and by the
        # discriminators' passes (parameters only); without sharing the flags are no-ops
        # (inputs=...: the engine then runs only the nodes that lead to those tensors, so the
        # discriminators' passes never enter the generator graph)
        batched = shared and self.opt["batched_D"]
        if self.loss_scaler is not None:
            # the passes differentiate scale * loss (a device operand: no sync); the callers' losses stay unscaled
            k = self.loss_scaler.scale_tensor
            loss_G, loss_D, loss_D_T = loss_G * k, loss_D * k, [l * k for l in loss_D_T]
        with autograd.backward_flags([self.netD] if shared else [], autograd.SKIP_PARAM_GRADS, 2 if batched else None), \
                autograd.backward_flags(self.netD_T if shared else [], autograd.SKIP_PARAM_GRADS, 1 if batched else None):
            loss_G.backward(retain_graph=shared, inputs=g_inputs)
        self.grads_G.all_reduce_async(self.world)
        if self._early_on:           # (the next window's FlowNet2 may start from here on, see reference_flows)
            if self._backward_done is None:
                self._backward_done = torch.cuda.Event()
            self._backward_done.record()
        with autograd.backward_flags(d_nets if shared else [], autograd.SKIP_INPUT_GRAD):
            if self.d_streams and shared and loss_D_T:
                # one pass over the three disjoint graphs: every node runs on the stream of its forward, so the
                # discriminators' passes overlap as their forwards did (separate backward() calls would each end with
                # the calling stream waiting for the pass, i.e. one discriminator after the other)
                params = list(self.grads_D.params)
                for s in range(len(loss_D_T)):
                    params += list(self.grads_DT[s].params)
                torch.autograd.backward([loss_D] + list(loss_D_T), inputs=params)
                self.grads_D.all_reduce_async(self.world)
                for s in range(len(loss_D_T)):
                    self.grads_DT[s].all_reduce_async(self.world)
            else:
                loss_D.backward(inputs=self.grads_D.params if shared else None)
                self.grads_D.all_reduce_async(self.world)
                for s, ld in enumerate(loss_D_T):
                    ld.backward(inputs=self.grads_DT[s].params if shared else None)
                    self.grads_DT[s].all_reduce_async(self.world)

    def optimizer_steps(self, n_temporal):
        """The three ``optimizer.step()`` of train_vid2vid.py:104-111, then one launch refreshing every packed weight."""
        scaler, guards = self.loss_scaler, self.grad_guards
        if guards is not None:       # (with or without a scaler: check, clip and step, or skip, per optimizer)
            by_opt = {id(g.optimizer): g for g in [guards["G"], guards["D"]] + guards["D_T"]}
            step = lambda o: o.step(scaler, by_opt[id(o)])  # noqa: E731
            self._stepped = [self.optimizer_G, self.optimizer_D] + self.optimizer_D_T[:n_temporal]
        else:
            step = (lambda o: o.step()) if scaler is None else (lambda o: o.step(scaler))  # noqa: E731
        # (world > 1: the averaged gradient is the same on every rank, so every rank takes the same skip decision)
        self.grads_G.wait()
        step(self.optimizer_G)
        if self.ema is not None:     # (world > 1: every rank averages the same parameters; no traffic)
            self.ema.update(self.optimizer_G)
        self.grads_D.wait()
        step(self.optimizer_D)
        for s in range(n_temporal):
            self.grads_DT[s].wait()
            step(self.optimizer_D_T[s])
        if scaler is not None:
            scaler.update([self.optimizer_G, self.optimizer_D] + self.optimizer_D_T[:n_temporal])
        # (after a skipped step this re-packs unchanged weights: correct, and not worth a device-side branch)
        if self.repacker is not None:
            self.repacker.run()          # every packed forward / data-gradient weight copy, one launch

    def train_window(self, input_A, input_B):
        """train_vid2vid.py:54-111 for one window.  Returns a dict of detached scalar losses: the totals ``G``, ``D``,
        ``D_T{s}`` and every term under the reference's names (``G_GAN`` ... ``W``; temporal ones with the scale
        appended, ``G_T_GAN0`` ...); with ``max_grad_norm`` also the gradient norm every stepped optimizer saw (``GN_G``,
        ``GN_D``, ``GN_D_T{s}``: views of the guards' device state, valid until the next window).  ``self.last_outputs`` keeps (fake_B, fake_B_raw, flow, weight), detached,
        ``self.last_inputs`` (real_A, real_B, flow_ref, conf_ref): what ``ir2rgb_amd.visuals`` draws a snapshot from."""
        fake_prev_last = self.fake_B_prev
        drop_grad_dsts()                    # (gradient destinations of the previous window's discriminator outputs)
        # The reference flows depend on real frames only (train_vid2vid.py:62-65 computes them after the generator, from
        # real_Bp = input_B[:, tG-2:]): FlowNet2 -- frozen, no autograd, replayed from a HIP graph from its third call at a
        # shape on -- runs on a second HIP stream BESIDE the generator forward and is joined before the losses that read
        # its result (-1.0 ms per window).  Calls that are not yet replays (eager warm-up, capture) run on the main
        # stream, before the generator: a capture has to own its stream.
        tG = self.opt["n_input_gen_frames"]
        real_Bp_in = input_B[:, tG - 2:]
        side = self._flow_stream(input_B)
        flow_ref, conf_ref, rb_s, extra_flows = self.reference_flows(real_Bp_in[:, 1:], real_Bp_in[:, :-1], side)
        ran_on = getattr(self.flow_net, "ran_on", None)
        _conv.SIDE_BUSY = ran_on is not None        # (per-launch timing brackets skip kernels that share the chip)
        fake_B, fake_B_raw, flow, weight, real_A, real_Bp = self.generate(input_A, input_B)
        _conv.SIDE_BUSY = False
        real_B_prev, real_B = real_Bp[:, :-1], real_Bp[:, 1:]
        if ran_on is not None:                      # FlowNet2 replayed on the side stream: join it here
            torch.cuda.current_stream(input_B.device).wait_stream(ran_on)
            for t in [flow_ref, conf_ref] + [x for pair in extra_flows.values() for x in pair] + [x for x in rb_s if x is not None]:
                t.record_stream(torch.cuda.current_stream(input_B.device))
        # compute_fake_B_prev (generator.py:283-287) AS THE REFERENCE'S LOOP EVALUATES IT.  train_vid2vid.py:60,:67-68
        # hands the previous window's pyramid LIST to model_g and afterwards to compute_fake_B_prev; in between,
        # generate_frame_train appends the new frames to the elements of that very list (generator.py:113, :175:
        # ``fake_B_pyr[si] = concat([fake_B_pyr[si], fake_B])`` on the caller's object).  So from the second window on
        # ``fake_B_last[0][:, -1:]`` is the frame generated in THIS window, and G_Warp compares fake_B with its own
        # flow_ref-warped copy.  Reproduced on purpose (pinned by tests/golden/window_*.npz, whose generating script
        # executes the reference's statements and therefore has the same aliasing); only the first window of a
        # sequence uses the given previous frame.
        fbp = real_B_prev[:, 0:1] if fake_prev_last is None else fake_B[:, -1:].detach()
        if fake_B.size(1) > 1:
            fbp = torch.cat([fbp, fake_B[:, :-1].detach()], 1)
        flat = lambda t: t.reshape((-1,) + tuple(t.shape[2:]))  # noqa: E731
        # (a reshape that has to copy is a launch: evaluated where image_losses is called, not here)
        image_args = lambda: [flat(t) for t in (real_B, fake_B, fake_B_raw, real_A, real_B_prev, fbp, flow, weight,  # noqa: E731
                                                flow_ref, conf_ref)]
        if SC.ENABLED:      # the losses read FlowNet2's results on this stream
            SC.consumed(flow_ref, "reference flow (FlowNet2 replay)"), SC.consumed(conf_ref, "flow confidence (FlowNet2 replay)")
        if self.d_streams:
            # The temporal discriminators first, each on its own stream (they wait for what the main stream has queued so
            # far: the generator and the frame bookkeeping), then the image discriminator on the main stream: four
            # independent networks of small layers side by side instead of one after the other.  The streams are joined
            # before the totals; the backward passes follow the forward streams (autograd), see backward_passes.
            rb_s, fb_s, fl_s, cf_s = self.skipped_frames(rb_s, extra_flows, fake_B, flow_ref, conf_ref)
            active = [s for s in range(self.t_scales) if rb_s[s] is not None]
            LT, joins = [], []
            for s in active:
                br = _Branch(rb_s[s], fb_s[s], fl_s[s], cf_s[s], slot=SLOT_D_TEMPORAL + s, force=True)
                with br:
                    lt = self.temporal_losses(s, rb_s[s], fb_s[s], fl_s[s], cf_s[s])
                LT.append(lt)
                joins.append((br, lt))
            L = self.image_losses(*image_args())
            for br, lt in joins:
                vec = getattr(lt, "vecs", None)
                br.join(*(list(lt.values()) + ([v for v in vec if v is not None] if vec else [])))
        else:
            L = self.image_losses(*image_args())
            rb_s, fb_s, fl_s, cf_s = self.skipped_frames(rb_s, extra_flows, fake_B, flow_ref, conf_ref)
            active = [s for s in range(self.t_scales) if rb_s[s] is not None]
            LT = [self.temporal_losses(s, rb_s[s], fb_s[s], fl_s[s], cf_s[s]) for s in active]
        loss_G, loss_D, loss_D_T = self.get_losses(L, LT)
        self.backward_passes(loss_G, loss_D, loss_D_T)
        self.optimizer_steps(len(loss_D_T))
        self.last_outputs = tuple(t.detach() for t in (fake_B, fake_B_raw, flow, weight))
        self.last_inputs = tuple(t.detach() for t in (real_A, real_B, flow_ref, conf_ref))     # (references: no copy)
        out = {"G": loss_G.detach(), "D": loss_D.detach()}
        out.update({f"D_T{s}": l.detach() for s, l in enumerate(loss_D_T)})
        out.update({k: v.detach() for k, v in L.items()})
        for s, lt in zip(active, LT):
            out.update({f"{k}{s}": v.detach() for k, v in lt.items()})
        if self.grad_guards is not None:    # the guards' device words: no launch, no copy
            out["GN_G"], out["GN_D"] = self.grad_guards["G"].norm_tensor, self.grad_guards["D"].norm_tensor
            out.update({f"GN_D_T{s}": self.grad_guards["D_T"][s].norm_tensor for s in range(len(loss_D_T))})
        return out


def synthetic_sequence(n_frames, h, w, seed, device, channels=3):
    """smooth random field (Gaussian noise, 15x15 box blur, tanh) translated by a
    per-sequence constant (dx,dy) in [-8,8]^2 px per frame.  Returns (A, B) [1, n_frames, C, H, W] in [-1,1]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    dx, dy = [int(v) for v in torch.randint(-8, 9, (2,), generator=g)]
    pad = 8 * n_frames + 8
    out = []
    for _ in range(2):
        base = torch.randn(1, channels, h + 2 * pad, w + 2 * pad, generator=g).to(device)
        base = torch.tanh(F.avg_pool2d(F.pad(base, (7, 7, 7, 7), mode="reflect"), 15, stride=1) * 6)
        frames = [base[:, :, pad + t * dy:pad + t * dy + h, pad + t * dx:pad + t * dx + w] for t in range(n_frames)]
        out.append(torch.stack(frames, 1).contiguous())
    return out[0], out[1]
