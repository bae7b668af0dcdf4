"""One flat fp32 gradient buffer per optimizer, all-reduced with RCCL in chunks -- early chunks while the backward pass
is still running (the data-parallel side of ir2rgb_amd.vid2vid)."""
import torch
import torch.distributed as dist

from . import autograd
from . import streamcheck as SC


class FlatGrads:
    """One flat fp32 gradient buffer per optimizer.  ``zero`` drops the .grad references, so the first
    contribution of a backward pass is adopted by autograd without an add kernel per parameter;
    ``all_reduce_async`` makes every .grad a view of the flat buffer and, for world > 1, issues a chunked
    RCCL all-reduce (~128 MB per collective) that AVERAGES (ReduceOp.AVG: no scaling pass over the buffer).
    A parameter that received no gradient gets a zero one, as the reference's zero_grad() + Adam step would
    see (train_vid2vid.py:93-105).

    ``direct=True`` (world > 1, every parameter used once per backward pass -- the generators): the convolutions
    write their weight gradients straight into their slices (ir2rgb_amd.autograd.GRAD_SINKS), so 99.9 % of the
    buffer is in place when the pass ends; the rest (biases, BatchNorm parameters, first / thin / padded layers) is
    gathered by one multi-tensor copy, as everything is when ``direct`` is off (the discriminators: several
    contributions per parameter and pass, summed by the autograd engine before they are adopted).  The in-place
    weights sit at the front of the buffer in parameter order, cut into chunks; a chunk goes onto the wire from the
    autograd hook of the parameter that completes it, i.e. WHILE the backward pass is still running (the generators'
    1.4 GB of residual-block gradients are produced over the last ~5 ms of their pass: the all-reduce then ends about
    when the pass does instead of starting there); ``all_reduce_async`` sends what is left.

    Streams: a collective is ordered after the stream that is current where it is issued, and nothing else.  After the
    pass that is every gradient (the engine joins the pass's streams before backward() returns).  Inside the pass a hook's
    stream is ordered after ITS parameter's gradient only, while the sinks of one chunk are written on the streams of their
    nodes -- two for a generator whose branches run on two streams (branch_streams_training): the hook first makes its
    stream wait for every other stream that wrote into the chunk (``_join_writers``)."""

    def __init__(self, params, chunk_elems=32 * 1024 * 1024, world=1, direct=False):
        self.params = [p for p in params if p.requires_grad]
        pad4 = lambda k: (k + 3) & ~3  # noqa: E731  every view starts on a 16-byte boundary (vector path of adam_kernel)
        n = sum(pad4(p.numel()) for p in self.params)
        dev = self.params[0].device
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.direct = bool(direct and world > 1)
        # layout: with ``direct`` the convolution weights (written in place by their weight-gradient kernels) come first,
        # in parameter order, so that whole chunks of the buffer are complete -- and can be all-reduced -- while the
        # backward pass is still running; biases / BatchNorm parameters (gathered by one copy when the pass ends) follow
        is_sink = [self.direct and p.dim() == 4 for p in self.params]
        order = [i for i, s in enumerate(is_sink) if s] + [i for i, s in enumerate(is_sink) if not s]
        self.views, off = [None] * len(self.params), 0
        starts = {}
        for i in order:
            p = self.params[i]
            starts[i] = off
            self.views[i] = self.flat[off:off + p.numel()].view_as(p)
            off += pad4(p.numel())
        self.chunk = chunk_elems
        self.handles = []
        self.scale_after = None
        # early chunks: [lo, hi) ranges of the sink region, each a list of parameter indices; a chunk is all-reduced from
        # the autograd hook of the parameter whose gradient completes it (all_reduce_async picks up what is left)
        self.chunks, self._fired, self._pending, self._issued, self._world = [], set(), [], [], world
        self._direct_capable, self._sink_ids, self._hooks = self.direct, [], []
        if self.direct:
            cur, lo = [], 0
            sink_ids = self._sink_ids = [i for i in order if is_sink[i]]
            for k, i in enumerate(sink_ids):
                cur.append(i)
                hi = starts[i] + pad4(self.params[i].numel())
                if hi - lo >= chunk_elems or k == len(sink_ids) - 1:
                    self.chunks.append((lo, hi, tuple(cur)))
                    cur, lo = [], hi
            self.sink_end = self.chunks[-1][1] if self.chunks else 0
            chunk_of = {i: c for c, (_, _, ids) in enumerate(self.chunks) for i in ids}
            for i in sink_ids:
                p = self.params[i]
                autograd.GRAD_SINKS[p] = self.views[i]
                self._hooks.append(p.register_post_accumulate_grad_hook(self._make_hook(i, chunk_of[i])))
        else:
            self.sink_end = 0

    def set_direct(self, on):
        """Arm / disarm the in-place sinks for the backward passes to come.  They are only sound while every parameter
        receives ONE contribution per pass: a window that generates several frames applies each generator several times,
        and a second contribution would overwrite the first in the same slice (autograd then sums two aliases of it) --
        the trainer switches to the gathered form for such windows (Vid2VidTrainer.generate)."""
        on = bool(on) and self._direct_capable
        if on == self.direct:
            return
        self.direct = on
        for i in self._sink_ids:
            if on:
                autograd.GRAD_SINKS[self.params[i]] = self.views[i]
            else:
                autograd.GRAD_SINKS.pop(self.params[i], None)
                autograd.SINK_STREAMS.pop(self.params[i], None)
        self._pending, self._issued = [], []

    def close(self):
        """Releases what this buffer holds on its parameters -- the in-place sinks, the post-accumulate hooks and the
        .grad views -- so that another FlatGrads can take them over (Vid2VidTrainer.update_fixed_params).  Outstanding
        all-reduces are waited for first."""
        self.wait()
        self.set_direct(False)
        for h in self._hooks:
            h.remove()
        self._hooks, self._sink_ids, self._direct_capable, self.chunks = [], [], False, []
        for p in self.params:
            p.grad = None

    def _make_hook(self, i, c):
        def hook(p):
            if not self._pending or i in self._fired:
                return
            self._fired.add(i)
            if p.grad is None or p.grad.data_ptr() != self.views[i].data_ptr():
                self._pending[c] = -1                      # this gradient is not in place: the chunk waits for the gather
                return
            if self._pending[c] > 0:
                self._pending[c] -= 1
                if self._pending[c] == 0:
                    lo, hi, _ = self.chunks[c]
                    self._join_writers(c)
                    self._reduce(lo, hi)
                    self._issued[c] = True
        return hook

    def _join_writers(self, c):
        """Chunk ``c`` is complete on the HOST: every weight-gradient kernel that writes into it has been queued, on the
        stream of its node (autograd.SINK_STREAMS).  The current stream -- the one the collective will be ordered after --
        waits for each of those that is not itself: at most the generators' branch stream in the trainer.  -> the streams
        it waited for (none where one stream wrote the whole chunk and runs the hook)."""
        writers = [autograd.SINK_STREAMS.get(self.params[i]) for i in self.chunks[c][2]]
        writers = [s for s in writers if s is not None]
        waited = []
        if writers:
            cur = torch.cuda.current_stream(writers[0].device)
            for s in writers:
                if s != cur and s not in waited:
                    waited.append(s)
                    cur.wait_stream(s)
        return waited

    def _reduce(self, lo, hi):
        if SC.ENABLED:      # the collective reads flat[lo:hi] after the current stream, and after nothing else
            SC.consumed_range(self.flat, lo, hi, "all-reduce range")
        avg = dist.get_backend() == "nccl"     # RCCL averages in the collective; gloo (CPU tests) has no AVG
        self.scale_after = None if avg else 1.0 / self._world
        for i in range(lo, hi, self.chunk):
            self.handles.append(dist.all_reduce(self.flat[i:min(i + self.chunk, hi)], op=dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM,
                                                async_op=True))

    def zero(self):
        for p in self.params:
            p.grad = None
        if self.direct:      # arm the early chunks for the backward pass that follows
            self._fired = set()
            self._pending = [len(ids) for _, _, ids in self.chunks]
            self._issued = [False] * len(self.chunks)

    def all_reduce_async(self, world):
        self._world = world
        src, dst, missing = [], [], []
        for p, v in zip(self.params, self.views):
            if p.grad is None:
                missing.append(v)
                p.grad = v
            elif world > 1 and p.grad.data_ptr() != v.data_ptr():
                src.append(p.grad)
                dst.append(v)
                p.grad = v
            elif world > 1:
                p.grad = v              # written in place by its convolution (GRAD_SINKS)
        issued, self._pending = self._issued, []           # (disarm the hooks)
        if missing:
            if any(issued):
                lo_hi = [(lo, hi) for (lo, hi, _), done in zip(self.chunks, issued) if done]
                base = self.flat.data_ptr()
                for v in missing:       # a parameter without gradient inside a chunk that is already on the wire cannot happen:
                    o = (v.data_ptr() - base) // 4          # its chunk never completes
                    assert not any(lo <= o < hi for lo, hi in lo_hi), "FlatGrads: early chunk reduced before it was complete"
            torch._foreach_zero_(missing)      # one multi-tensor launch instead of one fill per parameter
        if world <= 1:
            return
        if src:
            if SC.ENABLED:
                for t in src:
                    SC.consumed(t, "gathered gradient")
            torch._foreach_copy_(dst, src)
        # what the hooks have not sent: unfinished chunks of the sink region (merged into runs), then the gathered tail
        run = None
        for (lo, hi, _), done in zip(self.chunks, issued or [False] * len(self.chunks)):
            if done:
                if run is not None:
                    self._reduce(*run)
                    run = None
            else:
                run = (lo, hi) if run is None else (run[0], hi)
        tail_lo = self.sink_end
        if run is not None:
            tail_lo = run[0]
        self._reduce(tail_lo, self.flat.numel())
        self._issued = []

    def wait(self):
        for h in self.handles:
            h.wait()
        self.handles = []
        if self.scale_after is not None:
            self.flat.mul_(self.scale_after)
            self.scale_after = None
