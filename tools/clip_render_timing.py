"""The picture of a clip two ways, timed in alternation in one process: the per-frame loop (``render_frame`` per frame: three launches, a fresh output
and a scratch lookup each -- what ClipPipeline did before the draw list) against ONE ``render_clip`` call (whmr_mesh_render_draws: three launches
for the whole clip), at F = 8, 32, 64 frames of 720p with 1 and 4 persons per frame; and the strips of ``render_image_group`` per person against one
``render_clip_groups`` call.  Persons are body-sized ellipsoids of SMPL's vertex and face counts in front of the demo's pseudo-focal camera, resident
on the device.  A call is timed by the host clock around --calls back-to-back calls that end in a device synchronise (the loop is bound by launches,
not by the device: an enqueue time would hide exactly that); --rounds alternating windows, median and (min .. max).  Before anything is timed the two
paths are compared bit for bit.

    python tools/clip_render_timing.py [--rounds 7] [--calls 5] [--out profiles/clip_render_timing.txt] [--commit ID]
"""
import argparse
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from whmr_amd.demo import render_clip, render_frame
from whmr_amd.utils.renderer_cam import MeshRenderer, render_clip_groups, render_image_group

H, W = 720, 1280


def uv_sphere(rings=82, segments=84):
    """unit sphere with poles on the y axis: 2 + rings * segments = 6890 vertices, 2 * segments * rings = 13776 faces (SMPL's counts)"""
    th = np.pi * np.arange(1, rings + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones_like(ph)), np.outer(np.sin(th), np.sin(ph))], -1).reshape(-1, 3)
    verts = np.concatenate([[[0.0, 1.0, 0.0]], ring, [[0.0, -1.0, 0.0]]])
    at = lambda r, s: 1 + r * segments + s % segments
    faces = [[0, at(0, s + 1), at(0, s)] for s in range(segments)]
    for r in range(rings - 1):
        for s in range(segments):
            faces += [[at(r, s), at(r, s + 1), at(r + 1, s)], [at(r, s + 1), at(r + 1, s + 1), at(r + 1, s)]]
    last = 1 + rings * segments
    faces += [[last, at(rings - 1, s), at(rings - 1, s + 1)] for s in range(segments)]
    return verts, np.asarray(faces, dtype=np.int32)


def persons(n, rng, dev):
    """n ellipsoid persons (half axes 0.25 x 0.70 x 0.20 m) 2.5 .. 6 m in front of the camera, inside a 720p frame of focal sqrt(H^2 + W^2)"""
    sphere, _ = uv_sphere()
    verts = np.broadcast_to(sphere * np.array([0.25, 0.70, 0.20]), (n,) + sphere.shape).astype(np.float32)
    z = rng.uniform(2.5, 6.0, size=n)
    focal = math.sqrt(H * H + W * W)
    cam_t = np.stack([rng.uniform(-0.4, 0.4, size=n) * W * z / focal, rng.uniform(-0.2, 0.2, size=n) * H * z / focal, z], 1).astype(np.float32)
    return dict(local_smpl_vertices=torch.from_numpy(np.ascontiguousarray(verts)).to(dev), pred_cam_t=torch.from_numpy(cam_t).to(dev),
                focal_length=torch.full((n,), focal, dtype=torch.float32, device=dev))


def wall_ms(fn, n):
    """host milliseconds per call of n back-to-back calls of fn, the last one finished on the device"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def compare(old, new, rounds, calls):
    """(old, new) medians with their windows, alternating"""
    for fn in (old, new):
        for _ in range(2):
            fn()
    t = ([], [])
    for _ in range(rounds):
        t[0].append(wall_ms(old, calls))
        t[1].append(wall_ms(new, calls))
    return t


def fmt(v):
    return '%8.3f ms (%7.3f .. %7.3f)' % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=5, help='calls per timed window')
    ap.add_argument('--frames', type=int, nargs='+', default=[8, 32, 64])
    ap.add_argument('--persons', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_render_timing.txt'))
    ap.add_argument('--commit', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('clip_render_timing.py measures on a HIP device; none found')
    commit = a.commit
    if commit is None:
        r = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else 'unknown'
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    renderer = MeshRenderer(uv_sphere()[1])
    keys = ('local_smpl_vertices', 'pred_cam_t', 'focal_length')
    lines = ['command: python tools/clip_render_timing.py ' + ' '.join(sys.argv[1:]),
             'commit: %s   device: %s' % (commit, torch.cuda.get_device_name(0)),
             '720p frames and 6890-vertex persons on the device; host clock around %d calls ending in a synchronise, median of %d alternating windows '
             '(min .. max); every pair of paths compared bit for bit before it is timed' % (a.calls, a.rounds), '',
             'overlay of a clip: render_frame per frame (3 launches each)  |  one render_clip call (3 launches)  |  loop / clip']
    frames_all = torch.from_numpy(rng.integers(0, 256, size=(max(a.frames), H, W, 3), dtype=np.uint8)).to(dev)
    for F in a.frames:
        for P in a.persons:
            frames = frames_all[:F]
            out = persons(F * P, rng, dev)
            index = np.repeat(np.arange(F), P)

            def loop():
                return [render_frame({k: out[k][f * P:(f + 1) * P] for k in keys}, frames[f], renderer) for f in range(F)]

            def clip():
                return render_clip(out, frames, renderer, index)
            same = all(torch.equal(x, y) for x, y in zip(loop(), clip()))
            t = compare(loop, clip, a.rounds, a.calls)
            spread = max(max(v) - min(v) for v in t)
            lines.append('F = %2d, %d per frame: %s  |  %s  |  x %.2f   spread of a path %.3f ms   bits %s'
                         % (F, P, fmt(t[0]), fmt(t[1]), statistics.median(t[0]) / statistics.median(t[1]), spread, 'equal' if same else 'DIFFER'))
            del out
    lines += ['', 'strips (frame | overlay | side | side): render_image_group per person (9 launches, a zeros_like and a cat each)  |  one '
              'render_clip_groups call (3 launches)  |  loop / clip']
    for F, P in ((8, 1), (8, 4)):
        frames = frames_all[:F]
        out = persons(F * P, rng, dev)
        world = out['local_smpl_vertices'].flip(2).contiguous()                      # another orientation for the last panel
        index = np.repeat(np.arange(F), P)

        def loop():
            return [render_image_group(frames[index[p]], out['pred_cam_t'][p], world[p], out['local_smpl_vertices'][p], None, out['focal_length'][p:p + 1],
                                       (W // 2, H // 2), renderer) for p in range(F * P)]

        def clip():
            return render_clip_groups(frames, out['pred_cam_t'], world, out['local_smpl_vertices'], None, out['focal_length'], index, renderer)
        same = all(torch.equal(x, y) for x, y in zip(loop(), clip()))
        t = compare(loop, clip, a.rounds, a.calls)
        spread = max(max(v) - min(v) for v in t)
        lines.append('F = %2d, %d per frame: %s  |  %s  |  x %.2f   spread of a path %.3f ms   bits %s'
                     % (F, P, fmt(t[0]), fmt(t[1]), statistics.median(t[0]) / statistics.median(t[1]), spread, 'equal' if same else 'DIFFER'))
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
