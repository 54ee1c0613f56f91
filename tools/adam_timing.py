"""Optimizer step on the W-HMR parameter set (bf16 numerics), two ways, HIP events over windows of >= 0.3 s after warm-up, alternating:

  A  torch.optim.Adam(fused=True).step() + WeightOperands.refresh()     (what bench.py's training step does: update, then whmr_weights_prepare re-reads
                                                                         the ViT's 85 M matmul weights to write their bf16 W / W^T operand copies)
  B  whmr_amd.train.FusedAdam.for_model(model).step()                    (csrc/adam.hip: the update writes the copies itself)

Gradients are static random tensors, so neither side rebuilds its tables inside the window.  Prints the bytes each way has to move next to the
streaming-copy rate of this box (whmr_hbm_copy).

    python tools/adam_timing.py
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from whmr_amd import _lib as L
from whmr_amd.models import whmr_net
from whmr_amd.train import FusedAdam
from whmr_amd.train.vit_autograd import _weight_operands
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


ma, mb = model(), model()
vit = ma.feature_extractor.backbone
_weight_operands(vit)
wo = vit.__dict__['_train_operands']
adam = torch.optim.Adam(ma.parameters(), lr=5e-5, fused=True)
fused = FusedAdam.for_model(mb, lr=5e-5)
assert fused.operands is not None


def step_a():
    adam.step()
    wo.refresh()


def step_b():
    fused.step()


for _ in range(3):
    step_a()
    step_b()
torch.cuda.synchronize()
ta, tb = [], []
for _ in range(5):
    ta.append(timed(step_a))
    tb.append(timed(step_b))
n = sum(p.numel() for p in ma.parameters())
nw = sum(p.numel() for p in wo.params)
src, dst = torch.empty(1 << 28, dtype=torch.uint8, device=dev), torch.empty(1 << 28, dtype=torch.uint8, device=dev)
tc = timed(lambda: L._check(L.lib().whmr_hbm_copy(src.data_ptr(), dst.data_ptr(), src.numel(), L._stream()), 'whmr_hbm_copy'))
copy = 2 * src.numel() / tc
bytes_a, bytes_b = 28 * n + 8 * nw, 28 * n + 4 * nw
print('torch %s, %s' % (torch.__version__, torch.cuda.get_device_name(0)))
print('W-HMR, bf16 numerics: %d parameter tensors, %.1f M elements, of which %.1f M in the %d matmul weights of the ViT' % (len(list(ma.parameters())), n / 1e6, nw / 1e6, len(wo.params)))
print('A  torch fused Adam + whmr_weights_prepare : median %.1f us  (windows: %s)  %.2f GB -> copy floor %.1f us' % (
    statistics.median(ta) * 1e6, ' '.join('%.1f' % (t * 1e6) for t in ta), bytes_a / 1e9, bytes_a / copy * 1e6))
print('B  FusedAdam with attached operands        : median %.1f us  (windows: %s)  %.2f GB -> copy floor %.1f us' % (
    statistics.median(tb) * 1e6, ' '.join('%.1f' % (t * 1e6) for t in tb), bytes_b / 1e9, bytes_b / copy * 1e6))
print('streaming copy on this box: %.0f GB/s;  B / A = %.3f' % (copy / 1e9, statistics.median(tb) / statistics.median(ta)))
