"""The training objective at batch 64, forward + backward: the fused node (whmr_amd.train.objective.WHMRLossFn, csrc/whmr_loss.hip) against a float32
torch restatement of the same terms on the same device (tests/whmr_loss_reference.py: mask multiplication, no boolean gather -- the fastest form
eager torch offers; the reference's own methods additionally stop at the host for every mask).  Per configuration (default: 15 terms, everything
on: 24) it prints the device kernel launches of one call (torch.profiler), the eager time per call (HIP events over 50 calls, launch-bound) and
the time of the same call replayed from a captured graph (device time only).
   python tools/loss_timing.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch
from torch.profiler import ProfilerActivity, profile

import whmr_loss_reference as WR
from whmr_amd import _lib as L
from whmr_amd.train import WHMRLossFn

dev = torch.device('cuda:0')
B, V = 64, (6890, 1723, 431)


def launches(fn):
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [k.name for e in prof.events() for k in (getattr(e, 'kernels', None) or [])]
    return len(names), sum('loss_partial' in n or 'loss_finish' in n or 'loss_bwd' in n for n in names)


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


print('torch %s on %s' % (torch.__version__, torch.cuda.get_device_name(0)))
for name, all_on in (('default (15 terms)', False), ('everything on (24 terms)', True)):
    w = WR.ALL_ON_W if all_on else WR.DEFAULT_W
    rng = torch.Generator().manual_seed(0)
    preds, tgt = WR.make_case(B, V, 0, (torch.rand(B, generator=rng) < 0.7).double(), (torch.rand(B, generator=rng) < 0.5).double(), all_on=all_on,
                              dtype=torch.float32)
    pd, td = WR.to(preds, tgt, device=dev, requires_grad=True)
    flat = [p.get(k) for p in pd for k in L.LOSS_FIELDS]
    leaves = [t for t in flat if t is not None]
    nbytes = sum(t.numel() * 4 for t in leaves)

    def fused():
        losses = WHMRLossFn.apply(td, w, *flat)
        return torch.autograd.grad(losses.sum(), leaves)

    def restated():
        d = WR.loss_dict(pd, td, w)
        return torch.autograd.grad(torch.stack(list(d.values())).sum(), leaves)

    a, b = fused(), restated()
    err = max(((x - y).abs().max() / y.abs().max().clamp_min(1e-30)).item() for x, y in zip(a, b))
    print('%s, B = %d, %.1f MB of predictions; largest gradient difference between the two %.1e of the tensor' % (name, B, nbytes / 1e6, err))
    for label, fn in (('fused node        ', fused), ('torch restatement ', restated)):
        n, ours = launches(fn)
        print('  %s %4d device launches per call (%d of them csrc/whmr_loss.hip kernels, the rest torch: the sum of the terms and its backward) | '
              'eager %7.1f us | replayed graph %6.1f us' % (label, n, ours, timed(fn), timed(captured(fn))), flush=True)
