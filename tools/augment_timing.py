"""Time of one TrainBatchMaker call (csrc/augment.hip: taps, rotation, horizontal pass, vertical pass, labels) for a batch of 64 samples drawn from
three source image sizes, HIP events over a window of >= 0.3 s after warm-up, with the bytes the call has to move (every box read once, the
intermediate written and read once, the fp32 patches written) next to what a streaming copy of this box does (whmr_hbm_copy, the figure
bench.py --full reports as hbm_attainable_GBps).

    python tools/augment_timing.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from whmr_amd import _lib as L
from whmr_amd.datasets import TrainBatchMaker, draw_augm_params, draw_meta_mask
from whmr_amd.datasets.train_batch import crop_geometry

dev = torch.device('cuda:0')
B, N = 64, 4096
rng = np.random.RandomState(0)
sizes = ((480, 640), (720, 1280), (1080, 1920))
images = [torch.from_numpy(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).to(dev) for h, w in sizes]
img_of = rng.randint(0, 3, N)
wh = np.array([[sizes[i][1], sizes[i][0]] for i in img_of], dtype=np.float64)
lab = {'center': wh * rng.uniform(0.3, 0.7, (N, 2)), 'scale': wh[:, 1] * rng.uniform(0.35, 0.9, N) / 200.0,     # person boxes 0.35 .. 0.9 of the image height
       'pose': rng.normal(0, 0.3, (N, 72)), 'shape': rng.normal(0, 1, (N, 10)), 'part': np.concatenate([wh[:, None] * rng.uniform(0, 1, (N, 24, 2)), np.ones((N, 24, 1))], -1),
       'openpose': np.concatenate([wh[:, None] * rng.uniform(0, 1, (N, 25, 2)), np.ones((N, 25, 1))], -1), 'S': rng.normal(0, 0.4, (N, 24, 4)),
       'smpl_2dkps': np.concatenate([wh[:, None] * rng.uniform(0, 1, (N, 24, 2)), np.ones((N, 24, 1))], -1)}
maker = TrainBatchMaker(lab, dev)
idx = rng.randint(0, N, B)
params, mask = draw_augm_params(B, rng=rng), draw_meta_mask(B, rng=rng)
batch = [images[img_of[i]] for i in idx]
call = lambda: maker(batch, idx, params=params, meta_mask=mask)


def timed(fn, min_seconds=0.3):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 5
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


moved = 0
for b, i in enumerate(idx):
    ul, br, pad = crop_geometry(lab['center'][i], params[3][b] * lab['scale'][i], params[2][b])
    bw, bh = int(br[0] - ul[0]), int(br[1] - ul[1])
    box = (bw + 2 * pad) * (bh + 2 * pad) * 3 if params[2][b] != 0 else bw * bh * 3
    moved += box + (2 * bw * bh * 3 if params[2][b] != 0 else 0) + 2 * bh * 192 * 3 + 3 * 256 * 192 * 4
t = timed(call)
src, dst = torch.empty(1 << 28, dtype=torch.uint8, device=dev), torch.empty(1 << 28, dtype=torch.uint8, device=dev)
copy = lambda: L._check(L.lib().whmr_hbm_copy(src.data_ptr(), dst.data_ptr(), src.numel(), L._stream()), 'whmr_hbm_copy')
tc = timed(copy)
copy_gbps = 2 * src.numel() / tc / 1e9
print('torch %s, %s' % (torch.__version__, torch.cuda.get_device_name(0)))
print('TrainBatchMaker, batch %d from %s sources, %d samples rotated: %.1f us per call (host geometry + one table upload + 5 launches) = %.0f samples/s'
      % (B, ' / '.join('%dx%d' % (w, h) for h, w in sizes), int((params[2] != 0).sum()), t * 1e6, B / t))
print('bytes the call must move: %.1f MB -> %.1f GB/s; streaming copy on this box: %.0f GB/s; the copy floor of the call is %.1f us (%.1f x below the measured time)'
      % (moved / 1e6, moved / t / 1e9, copy_gbps, moved / (copy_gbps * 1e9) * 1e6, t / (moved / (copy_gbps * 1e9))))
