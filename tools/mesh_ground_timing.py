"""What the ground plane costs: ``render_clip_groups`` for a 16-person clip at 720 x 1280 (16 frames, one person each: 64 panels, 48 draws, one
launch group), timed three ways in alternation in one session -- the parent commit (a built checkout of it given with --parent; run twice, in two
processes, for its own run-to-run spread), this commit with ground=False and this commit with ground=True.  Each way runs in a worker process of its
own that keeps its tensors on the device; the driver asks the workers in turn for one window = --calls back-to-back calls ending in a device
synchronise, timed by the worker's host clock; --rounds windows each, median and (min .. max).  ground=False is today's entry point
(whmr_mesh_render_draws) and has to lie within the parent's own run-to-run spread; the ground=True figure (whmr_mesh_render_scene: 32 planes, 32
heights reduced on the device) is reported.  Before timing, each worker prints a checksum of its strips: ground=False has to give the parent's bytes.

    python tools/mesh_ground_timing.py [--parent DIR] [--rounds 9] [--calls 300] [--out profiles/mesh_ground_timing.txt] [--commit ID]
"""
import argparse
import hashlib
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, PERSONS = 720, 1280, 16


def worker(root, ground, calls):
    """serve windows from the package under ``root``: a line on stdin -> one timed window, its milliseconds per call on stdout"""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from whmr_amd.utils.renderer_cam import MeshRenderer, render_clip_groups
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from clip_render_timing import persons, uv_sphere
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, size=(PERSONS, H, W, 3), dtype=np.uint8)).to(dev)
    out = persons(PERSONS, rng, dev)
    # smpl_vertices: the same bodies leaning by a pitch of 15 degrees, so the last panel's floor lies elsewhere
    c, s = math.cos(math.radians(15.0)), math.sin(math.radians(15.0))
    world = (out['local_smpl_vertices'] @ torch.tensor([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]], device=dev).T).contiguous()
    renderer = MeshRenderer(uv_sphere()[1])
    index = list(range(PERSONS))
    kw = dict(ground=True) if ground else {}

    def call():
        return render_clip_groups(frames, out['pred_cam_t'], world, out['local_smpl_vertices'], None, out['focal_length'], index, renderer, **kw)
    for _ in range(5):
        strips = call()
    torch.cuda.synchronize()
    print('ready %s %s' % (hashlib.sha1(torch.stack(strips).cpu().numpy().tobytes()).hexdigest()[:16], torch.cuda.get_device_name(0).replace(' ', '_')), flush=True)
    for _ in sys.stdin:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        torch.cuda.synchronize()
        print('%.6f' % ((time.perf_counter() - t0) * 1e3 / calls), flush=True)


def fmt(v):
    return '%8.3f ms (%7.3f .. %7.3f), spread %.3f ms' % (statistics.median(v), min(v), max(v), max(v) - min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit (its package is imported from there)')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--calls', type=int, default=300, help='calls per timed window')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_ground_timing.txt'))
    ap.add_argument('--commit', default=None)
    ap.add_argument('--worker', nargs=2, metavar=('ROOT', 'GROUND'), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], a.worker[1] == '1', a.calls)
    commit = a.commit
    if commit is None:
        r = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else 'unknown'
    # the parent twice: two processes of the same code give its run-to-run spread in this session
    ways = ([('parent commit', a.parent, '0'), ('parent commit, again', a.parent, '0')] if a.parent else []) + [('this commit, ground=False', ROOT, '0'),
                                                                                                                ('this commit, ground=True', ROOT, '1')]
    procs, sums, device = [], [], '?'
    try:
        for name, root, ground in ways:                                      # one at a time: a worker is warm before the next one starts
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--calls', str(a.calls), '--worker', os.path.abspath(root), ground],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            procs.append(p)
            line = p.stdout.readline().split()
            if len(line) != 3 or line[0] != 'ready':
                sys.exit('the worker for "%s" did not start (a HIP device is needed)' % name)
            sums.append(line[1])
            device = line[2].replace('_', ' ')
        t = [[] for _ in ways]
        for _ in range(a.rounds):
            for k, p in enumerate(procs):
                p.stdin.write('go\n')
                p.stdin.flush()
                t[k].append(float(p.stdout.readline()))
    finally:
        for p in procs:
            p.stdin.close()
            p.wait(timeout=60)
    lines = ['command: python tools/mesh_ground_timing.py ' + ' '.join(sys.argv[1:]),
             'commit: %s   device: %s' % (commit, device),
             'render_clip_groups, %d persons in %d frames of %d x %d, 6890-vertex persons resident on the device: %d panels, %d draws, one launch group.'
             % (PERSONS, PERSONS, H, W, 4 * PERSONS, 3 * PERSONS),
             'One worker process per way, asked in turn; a window = %d calls ending in a synchronise, host clock; median of %d windows (min .. max).'
             % (a.calls, a.rounds), '']
    for (name, _, _), v, s in zip(ways, t, sums):
        lines.append('%-28s %s   strips sha1 %s' % (name, fmt(v), s))
    if a.parent:
        both = t[0] + t[1]
        lines += ['', 'ground=False: %.3f ms (median); the parent\'s two runs span %.3f .. %.3f ms (medians %.3f and %.3f); bytes %s'
                  % (statistics.median(t[2]), min(both), max(both), statistics.median(t[0]), statistics.median(t[1]), 'equal' if sums[0] == sums[2] else 'DIFFER')]
    lines.append('ground=True minus ground=False: %+.3f ms (median)' % (statistics.median(t[-1]) - statistics.median(t[-2])))
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
