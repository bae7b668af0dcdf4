"""Cost of the loss-scaled optimizer step at the generator's size: ir2rgb_grad_check +
ir2rgb_adam_step_checked (+ ir2rgb_loss_scale_update) against ir2rgb_adam_step on the same tensors.  The bytes predict
32 / 28 = 1.14 (one more read of the gradient); the check's two launches and the update are latency on top."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from ir2rgb_amd import optim as OP
dev = torch.device("cuda:0")
N_TENSORS, NUMEL = 155, 512 * 512 * 9           # 365.7 M parameters in residual-block sized tensors
params = [torch.nn.Parameter(torch.randn(NUMEL, device=dev) * 0.05) for _ in range(N_TENSORS)]
for p in params:
    p.grad = torch.randn(NUMEL, device=dev) * 0.01
n = N_TENSORS * NUMEL
opt = OP.FusedAdam(params)
scaler = OP.LossScaler(dev, init_scale=1.0)
def timeit(fn, reps=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3
def scaled():
    opt.step(scaler)
    scaler.update([opt])
plain_us = timeit(opt.step)
scaled_us = timeit(scaled)
plain2_us = timeit(opt.step)
print("plain  Adam step: %.1f M params, %.1f us, %.2f TB/s (28 B/param)" % (n / 1e6, plain_us, n * 28 / plain_us / 1e6))
print("scaled Adam step: check + step + update %.1f us, %.2f TB/s (32 B/param)" % (scaled_us, n * 32 / scaled_us / 1e6))
print("plain again: %.1f us;  ratio scaled / plain: %.3f (bytes: 1.143)" % (plain2_us, scaled_us / min(plain_us, plain2_us)))
print("skipped windows:", scaler.stats()["skipped"])
