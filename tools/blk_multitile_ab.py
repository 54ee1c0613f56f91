"""A/B of the multi-tile launches of the blocked bf16 GEMMs (whmr_gemm_blk_set_grid: -1 = one workgroup per tile, the parent's launches; 0 =
the default) on the eager forward as bench.py builds and times it, interleaved in ONE process on one box.
usage: python tools/blk_multitile_ab.py [--rounds 8] [--steps 100] [--warmup 5] [--b SETTING] [workload:batch ...]
       (default workloads: vit224:64 vit256x192:64 vitl256x192:32; --b: the setting of the B side, default 0)
One round of both sides runs first and is not counted (every shape warm, the package clock settled); a reading is `steps` forwards.
The bar (per workload): B faster in every round AND the median paired difference at least 3x the max - min spread of the A side's readings."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from whmr_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--steps', type=int, default=100)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--b', type=int, default=0)
ap.add_argument('workloads', nargs='*', default=['vit224:64', 'vit256x192:64', 'vitl256x192:32'])
opt = ap.parse_args()
dev = torch.device('cuda:0')
for spec in opt.workloads:
    name, batch = spec.split(':')
    args = bench.parse(['--workload', name, '--batch', batch])
    with torch.no_grad():
        step, _, _, _ = bench.build_workload(args, dev)
        a, b = [], []
        for rnd in range(-1, opt.rounds):
            L.lib().whmr_gemm_blk_set_grid(-1)
            ta = bench.time_steps(step, opt.steps, opt.warmup)
            L.lib().whmr_gemm_blk_set_grid(opt.b)
            tb = bench.time_steps(step, opt.steps, opt.warmup)
            if rnd >= 0:
                a.append(ta)
                b.append(tb)
            print('%s batch %s %s: one tile per workgroup %.4f ms   multi-tile (%d) %.4f ms   %+.1f us'
                  % (name, batch, 'round %d' % rnd if rnd >= 0 else 'warm-up round (not counted)', ta, opt.b, tb, (tb - ta) * 1e3), flush=True)
    L.lib().whmr_gemm_blk_set_grid(0)
    diff = [y - x for x, y in zip(a, b)]
    med, spread = statistics.median(diff) * 1e3, (max(a) - min(a)) * 1e3
    every = all(d < 0 for d in diff)
    print('%s batch %s: median paired difference %+.1f us (%.2f %% of %.4f ms); spread of the one-tile side %.1f us; faster in every round: %s; '
          'bar (every round faster and |median| >= 3 x spread): %s' % (name, batch, med, 100 * med / (statistics.median(a) * 1e3), statistics.median(a), spread,
                                                                         every, 'MET' if every and -med >= 3 * spread else 'NOT MET'), flush=True)
    del step
