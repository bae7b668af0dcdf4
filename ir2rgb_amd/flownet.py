"""Frozen FlowNet2 + confidence mask (models/flownet.py:20-57): the reference flow of the vid2vid loop, replayed from a
HIP graph once a shape is warm."""
import os

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import streamcheck as SC
from .ext import warp_diff_norm


class FlowNet(torch.nn.Module):
    """Frozen FlowNet2 + confidence mask (models/flownet.py)."""

    def __init__(self, conv_dtype=torch.bfloat16, seed=1, use_graph=None):
        super().__init__()
        from .flownet2_pytorch.models import FlowNet2
        self.use_graph = (os.environ.get("IR2RGB_FLOWNET_GRAPH", "1") != "0") if use_graph is None else bool(use_graph)
        self._graphs = {}   # shape key -> call count | (graph, in1, in2, (flow, conf)) | False (capture failed)
        self.ran_on = None  # the side stream the last call replayed on (None: it ran on the caller's stream)
        rng = torch.random.get_rng_state()
        torch.manual_seed(seed)  # no checkpoint offline: the reference's own init (models.py:68-77)
        self.flowNet = FlowNet2(conv_dtype=conv_dtype)
        torch.random.set_rng_state(rng)
        self.flowNet.eval()
        for p in self.flowNet.parameters():
            p.requires_grad_(False)

    @torch.no_grad()
    def forward(self, input_A, input_B, side=None):
        """``side``: a HIP stream a graph REPLAY of this call may run on (see Vid2VidTrainer.train_window); calls that
        still have lazy work to do (eager warm-up, capture) stay on the current stream.  ``self.ran_on`` tells which."""
        if input_A.dim() == 5:
            b, n, c, h, w = input_A.shape
            flow, conf = self.compute_flow_and_conf(input_A.reshape(-1, c, h, w), input_B.reshape(-1, c, h, w), side)
            return flow.view(b, n, 2, h, w), conf.view(b, n, 1, h, w)
        return self.compute_flow_and_conf(input_A, input_B, side)

    @staticmethod
    def _key(shape, im):
        return tuple(shape), im.dtype, str(im.device)

    def will_replay(self, n, im):
        """True when a call on ``n`` frame pairs shaped like ``im`` [., 3, H, W] would be a graph replay (no lazy work)."""
        return isinstance(self._graphs.get(self._key((n,) + tuple(im.shape[1:]), im)), tuple)

    def compute_flow_and_conf(self, im1, im2, side=None):
        """FlowNet2 is frozen, runs without autograd and with fixed shapes: ~330 small launches per call.
        After two eager calls at a shape the whole call (convolutions, operators, interpolations, the
        confidence mask) is captured into a HIP graph and replayed -- one launch, no host work between
        the kernels.  Any failure to capture falls back to the eager path for that shape (logged once)."""
        self.ran_on = None
        key = self._key(im1.shape, im1)
        ent = self._graphs.get(key)
        if not self.use_graph or not im1.is_cuda or ent is False:
            return self._flow_and_conf_eager(im1, im2)
        if ent is None or isinstance(ent, int):
            n = (ent or 0) + 1
            self._graphs[key] = n
            if n <= 2:
                return self._flow_and_conf_eager(im1, im2)
            try:
                a, b = im1.clone(), im2.clone()
                torch.cuda.synchronize(im1.device)
                g = torch.cuda.CUDAGraph()
                # (with a process group alive its watchdog thread polls events meanwhile: only this thread's calls are
                # subject to the capture rules then)
                mode = "thread_local" if dist.is_available() and dist.is_initialized() else "global"
                with torch.cuda.graph(g, capture_error_mode=mode):
                    out = self._flow_and_conf_eager(a, b)
                ent = self._graphs[key] = (g, a, b, out)
            except Exception as e:  # noqa: BLE001  capture is an optimisation, never a requirement
                self._graphs[key] = False
                print(f"[ir2rgb_amd] FlowNet2 graph capture failed at {key[0]} ({type(e).__name__}: {e}); staying eager",
                      flush=True)
                return self._flow_and_conf_eager(im1, im2)
        if side is None:
            return self._replay(ent, im1, im2)
        self.ran_on = side
        main = torch.cuda.current_stream(im1.device)
        if main == side:
            # the caller already works on the second stream (Vid2VidTrainer.reference_flows, resident inputs): no wait
            return self._replay(ent, im1, im2)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            out = self._replay(ent, im1, im2)
        for t in (im1, im2):
            t.record_stream(side)
        return out

    @staticmethod
    def _replay(ent, im1, im2):
        """One replay on the current stream: copy into the graph's inputs, replay, clone its outputs (the graph owns
        them: the next replay overwrites them)."""
        g, a, b, (flow, conf) = ent
        a.copy_(im1)
        b.copy_(im2)
        g.replay()
        out = flow.clone(), conf.clone()
        if SC.ENABLED:
            SC.produced(out[0], "reference flow (FlowNet2 replay)"), SC.produced(out[1], "flow confidence (FlowNet2 replay)")
        return out

    def _flow_and_conf_eager(self, im1, im2):
        assert im1.size(1) == 3 and im1.shape == im2.shape
        old_h, old_w = im1.shape[2:]
        new_h, new_w = old_h // 64 * 64, old_w // 64 * 64
        resize = old_h != new_h      # flownet.py:42 tests the height only ...
        if not resize and old_w != new_w:
            # ... and with a width that is not a multiple of 64 the reference dies in FlowNet2's torch.cat
            raise ValueError(f"FlowNet: width {old_w} is not a multiple of 64 while height {old_h} is "
                             "(the reference resizes only when the height is off, flownet.py:42)")
        if resize:
            im1 = F.interpolate(im1, size=(new_h, new_w), mode="bilinear")
            im2 = F.interpolate(im2, size=(new_h, new_w), mode="bilinear")
        flow = self.flowNet(torch.stack([im1, im2], dim=2)).float().contiguous()
        _, _, norm = warp_diff_norm(im1.float().contiguous(), im2.float().contiguous(), flow, want_warped=False,
                                    want_diff=False)
        conf = (norm * norm < 0.02).float()  # flownet.py:50,56-57: sum of squares < 0.02
        if resize:
            flow = F.interpolate(flow, size=(old_h, old_w), mode="bilinear") * old_h / new_h
            conf = F.interpolate(conf, size=(old_h, old_w), mode="bilinear")
        return flow, conf
