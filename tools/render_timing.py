"""Per-frame time of the mesh overlay renderer (MeshRenderer.render, csrc/mesh_render.hip) at 1280x720, 1920x1080 and 3840x2160 for 1, 4 and 16 persons
of SMPL size (a 6890-vertex / 13776-face sphere mesh scaled to a body-sized ellipsoid), `close` (a person fills about half the frame height) and `far`
(a person is about a twelfth of it), HIP events over a window of >= 0.3 s after warm-up -- and, next to it, the model call of FramePipeline (graph replay)
for the same person count on a 720p frame: the picture is only useful if it does not dominate the frame.

    python tools/render_timing.py [--quick]        # --quick: one short window per case (for a kernel trace)
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from whmr_amd.utils.renderer_cam import MeshRenderer

dev = torch.device('cuda:0')
quick = '--quick' in sys.argv


def sphere(rings=82, segments=84):
    th = np.pi * np.arange(1, rings + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones_like(ph)), np.outer(np.sin(th), np.sin(ph))], -1)
    v = np.concatenate([[[0.0, 1.0, 0.0]], ring.reshape(-1, 3), [[0.0, -1.0, 0.0]]])
    at = lambda r, s: 1 + r * segments + s % segments
    f = [(0, at(0, s + 1), at(0, s)) for s in range(segments)] + [(len(v) - 1, at(rings - 1, s), at(rings - 1, s + 1)) for s in range(segments)]
    for r in range(rings - 1):
        for s in range(segments):
            f += [(at(r, s), at(r, s + 1), at(r + 1, s)), (at(r, s + 1), at(r + 1, s + 1), at(r + 1, s))]
    return v, np.asarray(f, dtype=np.int32)


def timed(fn, min_seconds):
    """mean device time of fn() in microseconds over a window of at least min_seconds (HIP events), after warm-up"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, total = 5, 0.0
    while True:
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        total = e0.elapsed_time(e1) * 1e-3
        if total >= min_seconds or quick:
            return total / reps * 1e6
        reps = int(reps * max(2.0, 1.2 * min_seconds / max(total, 1e-6)))


v, faces = sphere()
body = (v * np.array([0.25, 0.85, 0.20])).astype(np.float32)                       # 1.7 m tall
renderer = MeshRenderer(faces)
rng = np.random.default_rng(0)
print('torch %s, %s' % (torch.__version__, torch.cuda.get_device_name(0)), flush=True)
print('mesh overlay: MeshRenderer.render, all persons in one depth buffer; covered = share of the frame drawn', flush=True)
for (W, H) in ((1280, 720), (1920, 1080), (3840, 2160)):
    focal = math.hypot(H, W)
    frame = torch.from_numpy(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).to(dev)
    for P in (1, 4, 16):
        for name, share in (('close', 0.5), ('far', 1.0 / 12)):
            tz = focal * 1.7 / (share * H)                                           # the 1.7 m body spans `share` of the frame height
            # persons spread over the frame width (neighbours overlap when close), staggered in depth
            u = (np.arange(P) + 0.5) / P * W - W / 2 if P > 1 else np.zeros(1)
            z = tz * (1 + 0.04 * (np.arange(P) % 3))
            cam_t = np.stack([u * z / focal, np.zeros(P), z], 1).astype(np.float32)
            verts = torch.from_numpy(np.broadcast_to(body, (P,) + body.shape).copy()).to(dev)
            ct, fl = torch.from_numpy(cam_t).to(dev), torch.full((P,), focal, device=dev)
            out = renderer.render(frame, verts, ct, fl, want=('face',))
            covered = (out['face'] >= 0).float().mean().item()
            us = timed(lambda: renderer.render(frame, verts, ct, fl), 0.3)
            print('%4dx%-4d %2d persons %-5s: %8.1f us / frame   (covered %.3f)' % (W, H, P, name, us, covered), flush=True)

if not quick:
    from whmr_amd.demo import FramePipeline
    from whmr_amd.models import whmr_net
    from whmr_amd.utils import synth
    assets = synth.make_assets(0)
    sd = synth.make_state_dict(0, assets)
    m = whmr_net(None, assets=assets, numerics='bf16')
    m.load_state_dict(sd, strict=False)
    m = m.to(dev).eval()
    frame = torch.from_numpy(rng.integers(0, 256, size=(720, 1280, 3), dtype=np.uint8)).to(dev)
    for P in (1, 4, 16):
        dets = [(float(rng.uniform(200, 1080)), float(rng.uniform(150, 570)), s, s) for s in rng.uniform(120, 400, size=P)]
        plain, drawn = FramePipeline(m), FramePipeline(m, renderer=renderer)
        a = timed(lambda: plain(frame, dets), 0.3)
        b = timed(lambda: drawn(frame, dets), 0.3)
        print('FramePipeline 1280x720 %2d persons: model call (crops + graph replay) %8.1f us / frame; with a picture of the synthetic model\'s vertices under the sphere\'s face table '
              '(a soup of frame-sized triangles: a worst case, not a body) %8.1f us' % (P, a, b), flush=True)
