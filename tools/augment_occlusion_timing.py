"""Time of one TrainBatchMaker call without and with synthetic occluders (stage 4a of csrc/augment.hip), on the batch of tools/augment_timing.py:
64 samples drawn from three source image sizes, HIP events over a window of >= 0.3 s after warm-up.  The bank holds 64 random RGBA objects of
60 .. 200 px a side; the pastes come from ``draw_occlusions`` (1 .. 7 per sample, factors 0.2 .. 1).  Every figure is the median of several
windows with their lowest and highest next to it (the run-to-run spread), and the windows of the two calls alternate.

    python tools/augment_occlusion_timing.py [--parent-tree DIR]

--parent-tree: a built checkout of the parent commit.  Its bank-less call is then timed too, by the same code in a child process of its own, in
turn with a child process of this tree (two rounds each), so that all three figures come from one box in one session.
"""
import argparse
import json
import os
import random
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--parent-tree', default=None)
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help=argparse.SUPPRESS)
ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
ap.add_argument('--windows', type=int, default=7)
args = ap.parse_args()


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def child():
    """the measurements one tree can make -> one JSON line"""
    sys.path.insert(0, args.tree)
    import numpy as np
    import torch
    from whmr_amd import datasets as D
    dev = torch.device('cuda:0')
    B, N = 64, 4096
    rng = np.random.RandomState(0)
    sizes = ((480, 640), (720, 1280), (1080, 1920))
    images = [torch.from_numpy(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).to(dev) for h, w in sizes]
    img_of = rng.randint(0, 3, N)
    wh = np.array([[sizes[i][1], sizes[i][0]] for i in img_of], dtype=np.float64)
    lab = {'center': wh * rng.uniform(0.3, 0.7, (N, 2)), 'scale': wh[:, 1] * rng.uniform(0.35, 0.9, N) / 200.0,
           'pose': rng.normal(0, 0.3, (N, 72)), 'shape': rng.normal(0, 1, (N, 10)),
           'part': np.concatenate([wh[:, None] * rng.uniform(0, 1, (N, 24, 2)), np.ones((N, 24, 1))], -1),
           'openpose': np.concatenate([wh[:, None] * rng.uniform(0, 1, (N, 25, 2)), np.ones((N, 25, 1))], -1), 'S': rng.normal(0, 0.4, (N, 24, 4)),
           'smpl_2dkps': np.concatenate([wh[:, None] * rng.uniform(0, 1, (N, 24, 2)), np.ones((N, 24, 1))], -1)}
    idx = rng.randint(0, N, B)
    params, mask = D.draw_augm_params(B, rng=rng), D.draw_meta_mask(B, rng=rng)
    batch = [images[img_of[i]] for i in idx]
    plain = D.TrainBatchMaker(lab, dev)
    calls = {'plain': lambda: plain(batch, idx, params=params, meta_mask=mask)}
    info = {}
    if hasattr(D, 'OccluderBank'):
        bank = [rng.randint(0, 256, size=(rng.randint(60, 201), rng.randint(60, 201), 4)).astype(np.uint8) for _ in range(64)]
        occ = D.draw_occlusions(B, len(bank), rng=rng, pyrng=random.Random(0))
        maker = D.TrainBatchMaker(lab, dev, occluders=bank)
        calls['occluded'] = lambda: maker(batch, idx, params=params, meta_mask=mask, occlusions=occ)
        from whmr_amd.datasets.train_batch import plan_occlusions
        rows, _ = plan_occlusions(occ, maker.bank.sizes)
        # per kept paste: destination pixels inside the kept columns and rows, and the source texels each of them averages (per axis ~ 1 / factor + 1)
        px = tex = 0
        for k, nw, nh, sx, sy in rows.tolist():
            h, w = maker.bank.sizes[k]
            n = max(0, min(sx + nw, 224) - max(sx, 32)) * max(0, min(sy + nh, 256) - max(sy, 0))
            px, tex = px + n, tex + n * (int(np.ceil(w / nw)) + 1) * (int(np.ceil(h / nh)) + 1)
        info = dict(pastes_drawn=int(sum(len(o) for o in occ)), pastes_kept=len(rows), pixels_blended=px, texel_reads_upper=tex,
                    pixels_of_batch=B * 256 * 192)

    def window(fn, min_seconds=0.3):
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

    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.windows):
        for k, fn in calls.items():
            times[k].append(window(fn) * 1e6)
    print(json.dumps(dict(times=times, info=info, torch=torch.__version__, device=torch.cuda.get_device_name(0))), flush=True)


def run_child(tree):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--tree', tree, '--windows', str(args.windows)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=240).stdout
    return json.loads(out.strip().splitlines()[-1])


if args.child:
    child()
    sys.exit(0)

runs = []
for r in range(2 if args.parent_tree else 1):
    runs.append(('this', run_child(args.tree)))
    if args.parent_tree:
        runs.append(('parent', run_child(os.path.abspath(args.parent_tree))))
first = runs[0][1]
print('torch %s, %s; batch 64, %d windows of >= 0.3 s per figure and process; us per call: median (lowest .. highest)' % (first['torch'], first['device'], args.windows))
fmt = lambda v: '%.1f (%.1f .. %.1f)' % stats(v)
for name, res in runs:
    print('  process of %-6s tree: ' % name + ', '.join('%s %s' % (k, fmt(v)) for k, v in res['times'].items()))
pool = lambda who, key: [t for name, res in runs if name == who for t in res['times'][key]]
plain, occluded = pool('this', 'plain'), pool('this', 'occluded')
print('this commit, without occluders: %s us' % fmt(plain))
if args.parent_tree:
    parent = pool('parent', 'plain')
    print('parent commit, same call:       %s us' % fmt(parent))
    lo, hi = min(parent), max(parent)
    print('  median of this commit %.1f us %s the parent\'s own spread %.1f .. %.1f us' % (stats(plain)[0], 'lies within' if lo <= stats(plain)[0] <= hi else 'LIES OUTSIDE', lo, hi))
print('this commit, with occluders:    %s us' % fmt(occluded))
cost = stats(occluded)[0] - stats(plain)[0]
i = first['info']
print('  the occluders cost %.1f us per call (%.0f %% of the call without them): %d of %d drawn pastes kept, %d pixel blends = %.2f per pixel of the batch\'s %d,'
      % (cost, 100 * cost / stats(plain)[0], i['pastes_kept'], i['pastes_drawn'], i['pixels_blended'], i['pixels_blended'] / i['pixels_of_batch'], i['pixels_of_batch']))
print('  at most %.1f M source texels read (4 bytes each, %.1f per blend)' % (i['texel_reads_upper'] / 1e6, i['texel_reads_upper'] / max(i['pixels_blended'], 1)))
