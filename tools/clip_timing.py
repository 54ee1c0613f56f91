"""Frames per second of clip inference (whmr_amd.demo.ClipPipeline: all persons of F frames in one model call) against a FramePipeline loop over the
same frames, one person per 720p frame, frames resident on the device (an offline clip, decoded ahead).  FramePipeline is what the package had before
ClipPipeline, so the loop stands for the per-frame path.  The two are timed in alternation, --rounds times each, and the median is reported with the
spread; the input preparation (crops + camera input, no model call) is timed the same way and reported as its share.

    python tools/clip_timing.py [--frames 1 8 32 64] [--rounds 5] [--out profiles/clip_timing.txt] [--commit ID]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from whmr_amd.demo import ClipPipeline, FramePipeline, prepare_clip, prepare_frame
from whmr_amd.models import whmr_net
from whmr_amd.utils import synth


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='+', default=[1, 8, 32, 64])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--clips', type=int, default=4, help='clips per timed window')
    ap.add_argument('--numerics', default='bf16')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_timing.txt'))
    ap.add_argument('--commit', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('clip_timing.py measures on a HIP device; none found')
    commit = a.commit
    if commit is None:
        r = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else 'unknown'
    dev = torch.device('cuda:0')
    assets = synth.make_assets(0)
    m = whmr_net(None, assets=assets, numerics=a.numerics)
    m.load_state_dict(synth.make_state_dict(0, assets), strict=False)
    m = m.to(dev).eval()
    rng = np.random.default_rng(0)
    lines = ['command: python tools/clip_timing.py ' + ' '.join(sys.argv[1:]), 'commit: %s   device: %s   numerics: %s' % (commit, torch.cuda.get_device_name(0), a.numerics),
             '720p frames on the device, one person per frame; median of %d alternating rounds of %d clips each (min .. max)' % (a.rounds, a.clips), '',
             '%3s | %-30s | %-30s | %-7s | %-22s | %-22s' % ('F', 'ClipPipeline frames/s', 'FramePipeline loop frames/s', 'ratio', 'clip input prep ms/frame', 'loop input prep ms/frame')]
    frame_pipe = FramePipeline(m)
    for F in a.frames:
        frames = torch.from_numpy(rng.integers(0, 256, size=(F, 720, 1280, 3), dtype=np.uint8)).to(dev)
        dets = [[(float(rng.uniform(200, 1080)), float(rng.uniform(150, 570)), s, s)] for s in rng.uniform(120, 400, size=F)]
        clip_pipe = ClipPipeline(m, person_bucket=8)
        clip = lambda: [clip_pipe(frames, dets) for _ in range(a.clips)]
        loop = lambda: [frame_pipe(frames[f], dets[f]) for _ in range(a.clips) for f in range(F)]
        clip_prep = lambda: [prepare_clip(frames, dets, True, 8) for _ in range(a.clips)]
        loop_prep = lambda: [prepare_frame(frames[f], dets[f]) for _ in range(a.clips) for f in range(F)]
        for fn in (clip, loop, clip_prep, loop_prep):                               # warm-up: graph capture, tap tables, allocator
            fn()
            fn()
        t = {k: [] for k in ('clip', 'loop', 'clip_prep', 'loop_prep')}
        for _ in range(a.rounds):                                                   # interleaved: the four share whatever else the host is doing
            t['clip'].append(timed(clip))
            t['loop'].append(timed(loop))
            t['clip_prep'].append(timed(clip_prep))
            t['loop_prep'].append(timed(loop_prep))
        n = a.clips * F
        fps = lambda k: '%8.1f (%.1f .. %.1f)' % (n / statistics.median(t[k]), n / max(t[k]), n / min(t[k]))
        ms = lambda k, whole: '%.3f (%2.0f %% of the call)' % (1e3 * statistics.median(t[k]) / n, 100 * statistics.median(t[k]) / statistics.median(t[whole]))
        ratio = statistics.median(t['loop']) / statistics.median(t['clip'])
        lines.append('%3d | %-30s | %-30s | %6.2fx | %-22s | %-22s' % (F, fps('clip'), fps('loop'), ratio, ms('clip_prep', 'clip'), ms('loop_prep', 'loop')))
        print(lines[-1], flush=True)
        del clip_pipe, frames
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
