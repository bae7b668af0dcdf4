"""Every convolution and BatchNorm launch of the 512 x 1024 training window, replayed at its recorded geometry against
fp64.

One test per entry of tests/window_geometries.json (oracle/window.py records it; test_window_manifest_fresh keeps it
current), through oracle/replay_kernels.py, each run in bf16 and f16 from one fp64 reference: operands are drawn on
values exact in both formats.  Per-element bounds are oracle/bounds.py's, fixed before anything runs.  Forward-type
launches go through the entry the window used (conv2d_fwd with its split-K workspace, or conv2d_fwd_view on
channel-slice buffers), with the recorded bias / statistics arguments; weight gradients through conv2d_wgrad, plain and
accumulating onto a seeded base; BatchNorm (finalize, fused finalize + apply, apply, backward) at its recorded rows /
channels / pixel count / activation / residuals / accumulation, against oracle/bn_ref.py.
Run with -s to see the per-launch worst err/bound table.
"""
import pytest

from oracle import replay
from oracle import replay_kernels as RK
from oracle import window as WG

CONV = WG.conv_entries()
FWD = [r for r in CONV if not r["entry"].startswith("wgrad")]
WGRAD = [r for r in CONV if r["entry"].startswith("wgrad")]
BN = WG.bn_entries()
BN_SHIFTED = [max((r for r in BN if r["entry"] == "ir2rgb_bn_finalize_ex"), key=lambda r: r["args"][3])]
TABLE = replay.Table()


@pytest.mark.gpu
@pytest.mark.parametrize("rec", FWD, ids=replay.ids(FWD))
def test_window_forward_launch(dev, rec):
    TABLE.run(WG.launch_id(rec), RK.replay_forward, dev, rec, kernel=rec["kernel"])


@pytest.mark.gpu
@pytest.mark.parametrize("rec", WGRAD, ids=replay.ids(WGRAD))
def test_window_wgrad_launch(dev, rec):
    TABLE.run(WG.launch_id(rec), RK.replay_wgrad, dev, rec, kernel=rec["kernel"])


@pytest.mark.gpu
def test_window_manifest_fresh(dev, monkeypatch):
    """The manifest is what the window launches now: a geometry it lacks, or an entry no longer launched, fails and
    is printed as the line to add or remove."""
    for k, v in WG.ENV.items():
        monkeypatch.setenv(k, v)
    recs, keys = WG.run_window(dev)
    man = WG.load()
    have = {WG.canon(r) for r in man["launches"]}
    now = {WG.canon(r) for r in recs}
    want_keys = {WG.prof_key(r) for r in man["launches"] if r["kind"] == "conv"}
    msg = []
    for line in sorted(now - have):
        msg.append("new (add to tests/window_geometries.json): " + line)
    for line in sorted(have - now):
        msg.append("no longer launched (remove): " + line)
    for k in sorted(keys ^ want_keys, key=str):
        msg.append(("_prof_key not in manifest: " if k in keys else "_prof_key no longer launched: ") + repr(k))
    assert not msg, "\n".join(msg)


@pytest.mark.gpu
@pytest.mark.parametrize("rec", BN, ids=replay.ids(BN))
def test_window_batchnorm_launch(dev, rec):
    TABLE.run(WG.launch_id(rec), RK.bn_case, dev, rec, False, kernel="batchnorm")


@pytest.mark.gpu
@pytest.mark.parametrize("rec", BN_SHIFTED, ids=[f"shifted-{i}" for i in replay.ids(BN_SHIFTED)])
def test_window_batchnorm_shifted_mean(dev, rec):
    """|mean| ~ 20 std: E[y^2] - E[y]^2 cancels; finalize, apply and backward at the window's largest BN geometry."""
    TABLE.run("shifted-" + WG.launch_id(rec), RK.bn_case, dev, rec, True, kernel="batchnorm")


def teardown_module(module):
    TABLE.report()
