"""Gradient sinks across streams: what a collective issued from an autograd hook may read.

On RCCL ranks the finer-scale generators run their two branches on two HIP streams, forward and -- through autograd --
backward; with one frame per window their weight-gradient kernels write straight into the flat all-reduce buffer
(autograd.GRAD_SINKS), each on the stream of its node; and the hook of the parameter that completes a chunk puts the chunk
on the wire, ordered after the stream that is current in that hook and after nothing else.  ir2rgb_amd.streamcheck tags
every sink write with its stream and checks the range a collective is about to read (FlatGrads._reduce); the hook makes
its stream wait for the other writers first (FlatGrads._join_writers).

The unit tests build the dangerous chunk directly -- two sinks, two streams, one chunk -- with no process group
(``_reduce`` replaced by the range check alone): ordered with the wait, caught without it, and the gathered form.  The
trainer test runs the shipped configuration on RCCL with one rank in a child process.  Everything asserted from the
vector clocks is deterministic: host-side bookkeeping of the calls this process makes, no timing involved."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

pytestmark = pytest.mark.gpu

WSHAPE = (64, 64, 3, 3)
WELEMS = 64 * 64 * 3 * 3


@pytest.fixture
def SC():
    from ir2rgb_amd import streamcheck
    streamcheck.enable()
    try:
        yield streamcheck
    finally:
        streamcheck.disable()


def _two_sinks_two_streams(dev, monkeypatch, SC, direct=True):
    """Two 64->64 3x3 convolution stages on a 1x64x16x32 input (the smallest the MFMA weight-gradient kernel takes without
    padding), stage 0 on the main stream and stage 1 on the generators' branch stream, their weights the two sinks of ONE
    chunk of a FlatGrads; ``_reduce`` performs the stream check's range check and records, no collective.  One backward
    pass, then ``all_reduce_async``.  -> (FlatGrads, recorded calls, the two sinks' tags as the pass left them)."""
    from ir2rgb_amd import autograd as A
    from ir2rgb_amd import conv as C
    from ir2rgb_amd import networks as N
    from ir2rgb_amd.flatgrads import FlatGrads
    dt = torch.bfloat16
    gen = torch.Generator().manual_seed(11)
    convs = [nn.Conv2d(64, 64, 3, 1, 0).to(dev) for _ in range(2)]
    bns = [nn.BatchNorm2d(64).to(dev) for _ in range(2)]
    with torch.no_grad():
        for c in convs:
            c.weight.copy_(torch.randn(WSHAPE, generator=gen) / 24.0)
    xs = [torch.randn(1, 64, 16, 32, generator=gen).to(dev).to(dt).contiguous(memory_format=torch.channels_last) for _ in range(2)]
    proj = [torch.randn(1, 64, 16, 32, generator=gen).to(dev) for _ in range(2)]
    fg = FlatGrads([c.weight for c in convs], chunk_elems=2 * WELEMS, world=2, direct=True)
    assert fg.direct and len(fg.chunks) == 1 and fg.chunks[0][:2] == (0, 2 * WELEMS) and set(fg.chunks[0][2]) == {0, 1}
    fg.set_direct(direct)
    calls = []

    def reduce_(self, lo, hi):
        rec = {"stream": torch.cuda.current_stream(dev).cuda_stream, "lo": lo, "hi": hi, "in_pass": bool(self._pending),
               "error": None}
        try:        # (never out of the autograd hook: the exception is kept for the test to look at)
            SC.consumed_range(self.flat, lo, hi, "all-reduce range")
        except SC.StreamOrderError as e:
            rec["error"] = e
        calls.append(rec)

    monkeypatch.setattr(FlatGrads, "_reduce", reduce_)
    try:
        stage = lambda i: A.conv_stage(xs[i], convs[i], bns[i], 1, C.PAD_REFLECT, dt, pad=1)  # noqa: E731
        fg.zero()
        z0 = stage(0)
        with N._Branch(xs[1], slot=N.SLOT_BRANCH, force=True) as br:
            z1 = stage(1)
        z1 = br.join(z1)
        loss = (z0.float() * proj[0]).sum() + (z1.float() * proj[1]).sum()
        loss.backward()
        tags = [SC.tag_of(v) for v in fg.views]
        # the pass has returned: the engine has joined its streams, the caller's stream may read every sink
        SC.consumed_range(fg.flat, 0, fg.flat.numel(), "the whole buffer after the pass")
        fg.all_reduce_async(2)
        torch.cuda.synchronize()
    finally:
        fg.set_direct(False)        # (the sinks are process-wide: autograd.GRAD_SINKS)
    fg.planned = [any(c.__dict__.get("_ir2rgb_plans", {}).values()) for c in convs]
    return fg, calls, tags


@pytest.mark.parametrize("path", ["planned", "general"])
def test_hook_orders_a_chunk_written_on_two_streams(dev, monkeypatch, SC, path):
    """One chunk, two sinks, written on two streams: the hook that completes the chunk issues ONE reduce over both slices,
    and the stream it is issued on is ordered after both writers.  Both places that write a sink are covered: the cached
    stage plan (what the trainer runs) and ConvStageFn's general path."""
    from ir2rgb_amd import stageplan
    monkeypatch.setattr(stageplan, "ENABLED", path == "planned")
    fg, calls, tags = _two_sinks_two_streams(dev, monkeypatch, SC)
    assert fg.planned == [path == "planned"] * 2
    in_pass = [c for c in calls if c["in_pass"]]
    assert len(in_pass) == 1 and (in_pass[0]["lo"], in_pass[0]["hi"]) == (0, 2 * WELEMS), calls
    # the premise, or the test proves nothing: both sinks are tagged as grad sinks, by two different streams
    assert all(t is not None and t[2] == f"grad sink {WSHAPE}" for t in tags), tags
    assert tags[0][0] != tags[1][0], tags
    assert [c["error"] for c in calls] == [None] * len(calls), calls
    # after the pass: what the hooks sent is not sent again, and the (empty) gathered tail passes the check on the caller's stream
    after = [c for c in calls if not c["in_pass"]]
    assert [(c["lo"], c["hi"]) for c in after] == [(2 * WELEMS, 2 * WELEMS)], calls
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(fg.params, fg.views))
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().sum()) > 0 for v in fg.views)


def test_without_the_hooks_wait_the_check_names_the_sink(dev, monkeypatch, SC):
    """The same pass with the hook's wait taken away: the range check raises, and names a gradient sink and its writer.
    (A host-side exception from the vector clocks: the kernels run as before.)  This is what the test above and the trainer
    test below would report if the wait were lost."""
    from ir2rgb_amd.flatgrads import FlatGrads
    monkeypatch.setattr(FlatGrads, "_join_writers", lambda self, c: [])
    fg, calls, tags = _two_sinks_two_streams(dev, monkeypatch, SC)
    in_pass = [c for c in calls if c["in_pass"]]
    assert len(in_pass) == 1 and tags[0][0] != tags[1][0], (calls, tags)
    err = in_pass[0]["error"]
    assert isinstance(err, SC.StreamOrderError), calls
    assert "grad sink" in str(err) and "no wait_stream" in str(err), err
    # (after the pass the engine's join orders the caller's stream after both writers: the helper's check of the whole
    # buffer passed, and so does all_reduce_async's)
    assert [c["error"] for c in calls if not c["in_pass"]] == [None], calls


def test_gathered_form_sends_nothing_from_the_hooks_and_passes_the_check(dev, monkeypatch, SC):
    """set_direct(False) (a window that applies the generators more than once): no sink, no reduce from a hook; the
    gradients are gathered after the pass, on the caller's stream, and reduced as one range -- which passes the check and
    holds bit for bit what the in-place form left in the buffer."""
    fg_d, calls_d, _ = _two_sinks_two_streams(dev, monkeypatch, SC)
    direct = fg_d.flat.clone()
    fg, calls, tags = _two_sinks_two_streams(dev, monkeypatch, SC, direct=False)
    assert not any(c["in_pass"] for c in calls), calls
    assert [(c["lo"], c["hi"], c["error"]) for c in calls] == [(0, fg.flat.numel(), None)], calls
    assert tags == [None, None]                    # nothing was written in place
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(fg.params, fg.views))
    assert torch.equal(fg.flat, direct) and float(direct.abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# trainer level: RCCL, one rank, a fresh child process
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


CHUNK = 2 * WELEMS      # two residual-block weights of the finer generator (64 -> 64, 3x3) per chunk


def _worker(rank, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    from ir2rgb_amd import streamcheck as SC
    from ir2rgb_amd import vid2vid as V
    SC.enable()
    tr = V.Vid2VidTrainer(dev, world_size=2, seed=0, first_layer_gen_filters=64, gen_blocks=2, resident_inputs=True,
                          n_scales_spatial=2, allreduce_chunk_elems=CHUNK)
    fg, g1 = tr.grads_G, tr.netG[1]
    res = {"branch_streams_training": bool(getattr(g1, "branch_streams_training", False)),
           "direct_capable": bool(fg._direct_capable), "backend": dist.get_backend(), "errors": [], "windows": []}
    # which sink belongs to which branch of netG[1], from the module: the label encoder, the flow decoder and its heads run
    # on the branch stream (CompositeLocalGeneratorModule.forward), the rest on the main stream
    side_mods = [g1.model_down_seg, g1.model_up_flow, g1.model_final_flow, g1.model_final_w]
    side_ids = {id(p) for m in side_mods for p in m.parameters()}
    g1_ids = {id(p) for p in g1.parameters()}
    branch = {i: ("side" if id(fg.params[i]) in side_ids else "main") for i in fg._sink_ids if id(fg.params[i]) in g1_ids}
    chunk_of = {(lo, hi): ids for lo, hi, ids in fg.chunks}
    orig_reduce, orig_join = V.FlatGrads._reduce, V.FlatGrads._join_writers
    state = {"reduces": [], "waits": 0}

    def join_(self, c):
        waited = orig_join(self, c)
        if self is fg:
            state["waits"] += len(waited)
        return waited

    def reduce_(self, lo, hi):
        if self is fg:
            rec = {"lo": lo, "hi": hi, "early": bool(self._pending), "stream": torch.cuda.current_stream(dev).cuda_stream,
                   "tags": {i: SC.tag_of(self.views[i]) for i in chunk_of.get((lo, hi), ())} if self._pending else {},
                   "wire": self.flat[lo:hi].clone()}          # on the stream the collective is ordered after
            state["reduces"].append(rec)
        try:
            return orig_reduce(self, lo, hi)
        except SC.StreamOrderError as e:      # (kept, not raised out of the autograd hook; the collective is then not issued)
            res["errors"].append(str(e))

    V.FlatGrads._reduce, V.FlatGrads._join_writers = reduce_, join_
    A, B = V.synthetic_sequence(5, 64, 128, 3, dev)
    for w in range(3):
        state["reduces"], state["waits"] = [], 0
        try:
            tr.train_window(A[:, w:w + 3], B[:, w:w + 3])
        except SC.StreamOrderError as e:
            res["errors"].append(str(e))
            break
        torch.cuda.synchronize()
        win = {"direct": bool(fg.direct), "waits": state["waits"], "n_early": 0, "early_elems": 0, "wire_equal": True,
               "early_streams_g1": [], "sink_streams_g1": {"main": set(), "side": set()}, "untagged_in_place": 0}
        for r in state["reduces"]:
            win["wire_equal"] &= bool(torch.equal(r["wire"], fg.flat[r["lo"]:r["hi"]]))
            if not r["early"]:
                continue
            win["n_early"] += 1
            win["early_elems"] += r["hi"] - r["lo"]
            win["untagged_in_place"] += sum(t is None or not t[2].startswith("grad sink") for t in r["tags"].values())
            g1_tags = {i: t for i, t in r["tags"].items() if i in branch and t is not None}
            if g1_tags:         # an early chunk with sinks of the finer generator: (branches, writer streams, hook stream)
                win["early_streams_g1"].append((sorted({branch[i] for i in g1_tags}), sorted({t[0][1] for t in g1_tags.values()}),
                                                r["stream"]))
        for i, b in branch.items():       # every in-place sink of netG[1], early or not: which stream wrote it
            t = SC.tag_of(fg.views[i])
            if t is not None and t[2].startswith("grad sink"):
                win["sink_streams_g1"][b].add(t[0][1])
        win["sink_streams_g1"] = {k: sorted(v) for k, v in win["sink_streams_g1"].items()}
        res["windows"].append(win)
    V.FlatGrads._reduce, V.FlatGrads._join_writers = orig_reduce, orig_join
    res["finite"] = all(bool(torch.isfinite(p).all()) for g in tr.netG for p in g.parameters())
    res["stats"] = dict(SC.STATS)
    SC.disable()
    torch.save(res, os.path.join(outdir, "sinks.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_trainer_windows_on_rccl_under_the_stream_check(tmp_path):
    """Three windows of the two-scale trainer told it is one of two RCCL ranks, under the stream check: the finer generator
    backward on two streams, sinks armed, early chunks on the wire from the hooks.

    Deterministic (vector clocks): (a) no StreamOrderError; (c) netG[1].branch_streams_training and the in-place sinks were
    on; both branches of netG[1] wrote sinks, on two different streams, and chunks holding sinks of EACH branch left from
    the hooks, every one of them ordered after all its writers.  Numerical companion, necessary but timing-dependent
    (a collective that overtook a writer may still have found the final values): what each reduce would have put on the
    wire -- a clone of its range on the stream the collective is ordered after -- equals the buffer's final contents bit
    for bit.

    What this configuration cannot produce is ONE early chunk holding sinks of BOTH branches: in the parameter order of
    CompositeLocalGeneratorModule every run of in-place sinks lies between two gathered weights (the x-expanded first
    layers, the separable heads: model_final_img sits between the image and the flow decoder), a chunk that contains a
    gathered weight waits for all_reduce_async, so every early chunk is written by one stream -- the ordering that keeps
    today's trainer safe even without the hook's wait.  The mixed chunk itself is held by the unit
    tests above; here ``mixed_early`` is reported, and checked like every other chunk if a layout change ever makes one."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mp.spawn(_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    res = torch.load(os.path.join(str(tmp_path), "sinks.pt"))
    print(res)
    assert res["backend"] == "nccl"
    assert res["errors"] == [], res["errors"]                                        # (a)
    assert res["branch_streams_training"] and res["direct_capable"], res             # (c)
    assert len(res["windows"]) == 3 and res["finite"], res
    for win in res["windows"]:
        assert win["direct"] and win["n_early"] > 0 and win["untagged_in_place"] == 0, win
        assert win["wire_equal"], win
        main, side = win["sink_streams_g1"]["main"], win["sink_streams_g1"]["side"]
        assert len(main) == 1 and len(side) == 1 and main != side, win              # two branches, two writer streams
        early = win["early_streams_g1"]
        assert any(b == ["main"] for b, _, _ in early) and any(b == ["side"] for b, _, _ in early), win
        mixed_early = sum(len(s) > 1 for _, s, _ in early)
        print(f"early chunks {win['n_early']}, of netG[1] {len(early)}, written by two streams {mixed_early}, "
              f"wait_stream calls from the hooks {win['waits']}")
    assert res["stats"]["cross_stream"] > 0, res["stats"]
