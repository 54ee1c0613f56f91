"""Device time of the smoothing stage (TrackSmoother.run: table upload + one whmr_track_smooth launch + two SMPL calls) beside ClipPipeline's model
call (the replayed HIP graph) at 32 frames x 4 tracks, 720p frames resident on the device.  Both are timed with device events on the pipeline's
stream, in alternation, --rounds windows of --clips calls each; the median per call is reported with the spread.  The filter launch alone is timed
the same way.  No gate: the parent of this stage has nothing to compare with; the numbers are recorded in docs/kernels.md.

    python tools/smooth_timing.py [--frames 32] [--tracks 4] [--rounds 7] [--clips 8] [--out profiles/smooth_timing.txt] [--commit ID]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from whmr_amd import _lib as L
from whmr_amd.demo import ClipPipeline, TrackSmoother
from whmr_amd.models import whmr_net
from whmr_amd.utils import synth


def event_ms(fn, n):
    """device milliseconds per call of n back-to-back calls of fn on the current stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--tracks', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--clips', type=int, default=8, help='calls per timed window')
    ap.add_argument('--numerics', default='bf16')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'smooth_timing.txt'))
    ap.add_argument('--commit', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('smooth_timing.py measures on a HIP device; none found')
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
    F, T = a.frames, a.tracks
    frames = torch.from_numpy(rng.integers(0, 256, size=(F, 720, 1280, 3), dtype=np.uint8)).to(dev)
    dets = [[(float(rng.uniform(200, 1080)), float(rng.uniform(150, 570)), s, s) for s in rng.uniform(120, 400, size=T)] for _ in range(F)]
    ids = [list(range(T)) for _ in range(F)]
    pipe = ClipPipeline(m, person_bucket=8)
    sm = TrackSmoother(m, max_tracks=max(64, T))
    out = pipe(frames, dets)                                                        # the rows the stage is timed on (static buffers of the graph)

    def model_call():
        pipe(frames, dets)                                                          # input preparation + replay: what a clip costs without smoothing

    def stage():
        sm.run(out, sm.plan_clip(dets, ids))

    plan = sm.plan_clip(dets, ids)
    table = torch.from_numpy(plan.table()).to(dev)
    state = sm._device_state(dev)
    ins = [out[k].float().contiguous() for k in ('local_pose', 'global_pose', 'pred_cam_t', 'focal_length', 'shape')]

    def launch():
        L.track_smooth(*ins, table, plan.T, plan.n_tracked, state, sm.min_cutoff, sm.beta, sm.d_cutoff)

    for fn in (model_call, stage, launch):                                          # warm-up: graph capture, code objects, allocator
        for _ in range(3):
            fn()
    t = {k: [] for k in ('model', 'stage', 'launch')}
    for _ in range(a.rounds):                                                       # interleaved: the three share whatever else the box is doing
        t['model'].append(event_ms(model_call, a.clips))
        t['stage'].append(event_ms(stage, a.clips))
        t['launch'].append(event_ms(launch, a.clips))
    fmt = lambda k: '%8.3f ms (%.3f .. %.3f)' % (statistics.median(t[k]), min(t[k]), max(t[k]))
    share = statistics.median(t['stage']) / statistics.median(t['model'])
    lines = ['command: python tools/smooth_timing.py ' + ' '.join(sys.argv[1:]),
             'commit: %s   device: %s   numerics: %s' % (commit, torch.cuda.get_device_name(0), a.numerics),
             '%d frames x %d tracks = %d rows, 720p frames on the device; device events, median of %d alternating windows of %d calls (min .. max)'
             % (F, T, F * T, a.rounds, a.clips), '',
             'ClipPipeline call without smoothing (input preparation + replayed graph): %s' % fmt('model'),
             'smoothing stage (table upload + filter launch + two SMPL calls):          %s   = %.1f %% of the call above' % (fmt('stage'), 100 * share),
             'whmr_track_smooth alone (one launch, %d wavefronts):                       %s' % (plan.T + plan.P - plan.n_tracked, fmt('launch'))]
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
