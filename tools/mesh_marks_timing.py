"""What keypoint skeletons and wireframe cost: ``render_clip`` for a 16-frame clip at 1080 x 1920 with 4 SMPL-sized persons per frame (64 draws into 16
images, one launch group), five ways timed in alternation in one process -- the plain call (whmr_mesh_render_draws: the entry and kernels it has
always used), wireframe, every person's 49-joint skeleton under the meshes, over the meshes, and wireframe with both (the last four through
whmr_mesh_render_marked).  Persons are body-sized ellipsoids of SMPL's vertex and face counts in front of the demo's pseudo-focal camera, their joints
49 points inside the ellipsoid, all resident on the device.  A window = --calls back-to-back calls between two HIP events on the stream, read after a
synchronise; --rounds windows per way, alternating (plain, wireframe, ..., plain, ...), median and (min .. max).  Nobody has measured these before:
there is no threshold, the figures are reported.  The last line is the box's shader clock as rocm-smi shows it right after the last window.

    python tools/mesh_marks_timing.py [--rounds 9] [--calls 50] [--out profiles/mesh_marks_timing.txt] [--commit ID]
"""
import argparse
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

from clip_render_timing import uv_sphere
from whmr_amd.utils.renderer_cam import MeshRenderer

H, W, FRAMES, PER_FRAME, JOINTS = 1080, 1920, 16, 4, 49


def clip(rng, dev):
    """FRAMES * PER_FRAME ellipsoid persons (half axes 0.25 x 0.70 x 0.20 m) 2.5 .. 6 m in front of the camera of focal sqrt(H^2 + W^2), each with
    JOINTS points inside its ellipsoid -> (verts, cam_t, focal, joints, frame_index)"""
    n = FRAMES * PER_FRAME
    sphere, _ = uv_sphere()
    radii = np.array([0.25, 0.70, 0.20])
    verts = np.broadcast_to(sphere * radii, (n,) + sphere.shape).astype(np.float32)
    z = rng.uniform(2.5, 6.0, size=n)
    focal = math.sqrt(H * H + W * W)
    cam_t = np.stack([rng.uniform(-0.4, 0.4, size=n) * W * z / focal, rng.uniform(-0.2, 0.2, size=n) * H * z / focal, z], 1).astype(np.float32)
    d = rng.normal(size=(n, JOINTS, 3))
    joints = (d / np.linalg.norm(d, axis=2, keepdims=True) * rng.uniform(size=(n, JOINTS, 1)) ** (1 / 3) * radii).astype(np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return up(verts), up(cam_t), torch.full((n,), focal, dtype=torch.float32, device=dev), up(joints), np.repeat(np.arange(FRAMES), PER_FRAME)


def window_ms(fn, calls):
    """device milliseconds per call of ``calls`` back-to-back calls, between two events on the stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def clock_line():
    try:
        r = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=30)
        sclk = [l.strip() for l in r.stdout.splitlines() if 'sclk' in l]
        return 'clock (rocm-smi --showclocks, first device): %s' % (sclk[0] if sclk else 'not shown')
    except (OSError, subprocess.TimeoutExpired):
        return 'clock: rocm-smi not available'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--calls', type=int, default=50, help='calls per timed window')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_marks_timing.txt'))
    ap.add_argument('--commit', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('mesh_marks_timing.py measures on a HIP device; none found')
    commit = a.commit
    if commit is None:
        r = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else 'unknown'
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, size=(FRAMES, H, W, 3), dtype=np.uint8)).to(dev)
    verts, cam_t, focal, joints, index = clip(rng, dev)
    r = MeshRenderer(uv_sphere()[1])
    ways = [('plain (whmr_mesh_render_draws)', {}),
            ('wireframe', dict(wireframe=True)),
            ('skeleton under', dict(joints=joints, keypoints_layer='under')),
            ('skeleton over', dict(joints=joints, keypoints_layer='over')),
            ('wireframe + skeleton under', dict(wireframe=True, joints=joints, keypoints_layer='under'))]
    calls = [lambda kw=kw: r.render_clip(frames, verts, cam_t, focal, index, **kw) for _, kw in ways]
    changed = []
    base = torch.stack(calls[0]())
    for fn in calls:
        for _ in range(3):
            out = fn()
        changed.append((torch.stack(out) != base).any(-1).float().mean().item())
    t = [[] for _ in ways]
    for _ in range(a.rounds):
        for k, fn in enumerate(calls):
            t[k].append(window_ms(fn, a.calls))
    lines = ['command: python tools/mesh_marks_timing.py ' + ' '.join(sys.argv[1:]),
             'commit: %s   device: %s' % (commit, torch.cuda.get_device_name(0)),
             'render_clip, %d frames of %d x %d, %d persons per frame (6890 vertices, 13776 faces, %d joints each) resident on the device: %d draws into %d '
             'images, one launch group of three.' % (FRAMES, H, W, PER_FRAME, JOINTS, FRAMES * PER_FRAME, FRAMES),
             'A window = %d calls between two HIP events; %d windows per way, alternating; median (min .. max); host work per call (planning and '
             'uploading the tables) is inside the window.' % (a.calls, a.rounds), '']
    plain = statistics.median(t[0])
    for (name, _), v, c in zip(ways, t, changed):
        lines.append('%-32s %8.3f ms (%7.3f .. %7.3f)   %+7.3f ms against plain   pixels changed against plain %.4f'
                     % (name, statistics.median(v), min(v), max(v), statistics.median(v) - plain, c))
    lines += ['', clock_line()]
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
