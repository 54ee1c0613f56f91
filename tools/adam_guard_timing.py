"""Cost of FusedAdam's gradient guard: the optimizer step on the W-HMR parameter set (bf16 numerics, the ViT's operands attached), HIP events over
windows of >= 0.3 s after warm-up, alternating:

  off  FusedAdam.for_model(model).step()                                          2 launches, 28 B per parameter (+ 4 B per matmul weight)
  on   FusedAdam.for_model(model, max_grad_norm=..., skip_nonfinite=True).step()  3 launches, the gradients read once more (+ 4 B per parameter)

The clip threshold is half the gradients' norm, so every guarded step clips; the gradients are static random tensors, so no table is rebuilt
inside a window.  On a tree whose FusedAdam has no guard only "off" is timed (the same file, copied there, gives the number to compare with).

    python tools/adam_guard_timing.py
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from whmr_amd.models import whmr_net
from whmr_amd.train import FusedAdam
from whmr_amd.utils import synth

dev = torch.device('cuda:0')
assets = synth.make_assets(0)
sd = synth.make_state_dict(0, assets)


def model():
    m = whmr_net(None, assets=assets, numerics='bf16')
    m.load_state_dict(sd, strict=False)
    m = m.to(dev).train()
    g = torch.Generator().manual_seed(1)
    for p in m.parameters():
        p.grad = (torch.randn(p.shape, generator=g) * 1e-3).to(dev)
    return m


def timed(fn, min_seconds=0.3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 20
    while True:
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        total = e0.elapsed_time(e1) * 1e-3
        if total >= min_seconds:
            return total / reps
        reps = int(reps * max(2.0, 1.2 * min_seconds / max(total, 1e-6)))


has_guard = hasattr(FusedAdam, 'set_grad_guard')
m_off = model()
n = sum(p.numel() for p in m_off.parameters())
steps = {'off': FusedAdam.for_model(m_off, lr=5e-5)}
if has_guard:
    norm = sum(float(p.grad.double().pow(2).sum()) for p in m_off.parameters()) ** 0.5
    steps['on'] = FusedAdam.for_model(model(), lr=5e-5, max_grad_norm=0.5 * norm, skip_nonfinite=True)
assert all(o.operands is not None for o in steps.values())
for _ in range(3):
    for o in steps.values():
        o.step()
torch.cuda.synchronize()
times = {k: [] for k in steps}
for _ in range(7):
    for k, o in steps.items():
        times[k].append(timed(o.step))
out = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'parameters': n, 'tensors': len(list(m_off.parameters())),
       'has_guard': has_guard}
for k, ts in times.items():
    out['%s_us' % k] = round(statistics.median(ts) * 1e6, 1)
    out['%s_windows_us' % k] = [round(t * 1e6, 1) for t in ts]
if has_guard:
    s = steps['on'].guard_summary()
    out.update(on_over_off=round(out['on_us'] / out['off_us'], 4), workgroups=steps['on']._blocks, guard=s)
    assert s['steps_skipped'] == 0 and s['clip_coef'] < 1.0
print(json.dumps(out))
