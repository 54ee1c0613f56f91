"""float64 numpy restatement of the checkerboard ground plane of the mesh renderer (whmr_mesh_render_scene), written from the plane's definition and the
reference call site (utils/renderer_cam.py:53,95-104: the plane lifted to mesh.bounds[0, 1], the mesh turned by the side view, the plane not), not
from the kernel.  Built on tests/mesh_render_reference.py for everything that concerns the mesh.  Test infrastructure: the package never imports it.
``dtype=np.float32`` runs the same arithmetic in single precision.

The plane: the horizontal square |q_x| <= half, |q_z| <= half at q_y = h in the renderer's world frame q = S D p (y up), n x n flat, unlit tiles, dark
where ix + iz is even.  h = the lowest world-frame y of the person's mesh = -max_v p_y (NaN vertices skipped), or given.  One image, one camera and
one plane per person."""
import numpy as np

import mesh_render_reference as MR

HALF, TILES = 2.0, 9
DARK, LIGHT = 35 / 255, 220 / 255


def lowest_point(verts, dtype=np.float64):
    """h of every person [P]: -max p_y over the vertices that are numbers, NaN for a mesh without one"""
    y = np.asarray(verts, dtype)[..., 1]
    some = ~np.isnan(y).all(axis=1)
    h = np.full(y.shape[0], np.nan, dtype)
    h[some] = -np.nanmax(y[some], axis=1)
    return h


def plane(H, W, cam_t, focal, center, rot, h, half=HALF, n=TILES, znear=MR.ZNEAR, dtype=np.float64):
    """One person's plane seen by that person's camera: (covers [H, W] bool, depth Z_g [H, W], ix, iz [H, W] int).  The camera is
    (X, Y, Z) = D R^T q + t, so q = R D ((X, Y, Z) - t); pixel (j, i) looks along (a, b, 1) Z with a = (i + 0.5 - cx) / fx, b = (j + 0.5 - cy) / fy:
    q = Z w + o with w = R D (a, b, 1), o = -R D t, and the plane q_y = h is met at Z_g = (h - o_y) / w_y."""
    t, f = np.asarray(cam_t, dtype), np.asarray(focal, dtype)
    R = np.eye(3, dtype=dtype) if rot is None else np.asarray(rot, dtype)
    RD = (R @ np.diag([1.0, -1.0, -1.0]).astype(dtype)).astype(dtype)
    a = ((np.arange(W, dtype=dtype) + dtype(0.5) - dtype(center[0])) / f[0])[None, :] * np.ones((H, 1), dtype)
    b = ((np.arange(H, dtype=dtype) + dtype(0.5) - dtype(center[1])) / f[1])[:, None] * np.ones((1, W), dtype)
    w = np.stack([a, b, np.ones_like(a)], -1) @ RD.T
    o = -(RD @ t)
    half, tile = dtype(half), dtype(2 * half) / dtype(n)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        Z = (dtype(h) - o[1]) / w[..., 1]
        qx, qz = Z * w[..., 0] + o[0], Z * w[..., 2] + o[2]
        fi, fk = np.floor((qx + half) / tile), np.floor((qz + half) / tile)
        covers = np.isfinite(Z) & (Z > dtype(znear)) & (fi >= 0) & (fi < n) & (fk >= 0) & (fk < n)
    ix, iz = np.where(covers, fi, 0).astype(np.int64), np.where(covers, fk, 0).astype(np.int64)
    return covers, Z.astype(dtype), ix, iz


def render(frame, verts, faces, cam_t, focal, center=None, rot=None, sideview_angle=0, ground=True, base=(0.65, 0.74, 0.86), colors=(DARK, LIGHT),
           half=HALF, n=TILES, znear=MR.ZNEAR, dtype=np.float64):
    """One image per person (``per_person=True`` of the renderer) with that person's plane.  ground: True = at the mesh's lowest point, a float = at
    that height, None = no plane (the mesh renderer's contract).  Returns dict(image uint8 [P, H, W, 3], color [P, H, W, 3], face [P, H, W] int32 (-1 on
    the plane and the background), ground [P, H, W] int32 (ix n + iz, -1 = no plane there), depth [P, H, W], ground_y [P]).  The plane owns a pixel
    iff it covers it and no face does or Z_g < the face's depth (a tie goes to the mesh)."""
    out = MR.render(frame, verts, faces, cam_t, focal, center=center, rot=rot, sideview_angle=sideview_angle, per_person=True, base=base, znear=znear,
                    dtype=dtype)
    H, W = frame.shape[:2]
    P = np.asarray(verts).shape[0]
    focal = np.asarray(focal, dtype).reshape(P, -1)
    focal = np.broadcast_to(focal, (P, 2)) if focal.shape[1] == 1 else focal
    center = (W // 2, H // 2) if center is None else center
    image, color, face, depth = out['image'].copy(), out['color'].copy(), out['face'].copy(), out['depth'].copy()
    tiles = np.full((P, H, W), -1, np.int32)
    ground_y = np.full(P, np.nan, dtype)
    if ground is not None:
        ground_y = lowest_point(verts, dtype) if ground is True else np.full(P, ground, dtype)
    for p in range(P):
        if np.isnan(ground_y[p]):
            continue
        covers, Z, ix, iz = plane(H, W, np.asarray(cam_t, dtype)[p], focal[p], center, rot, ground_y[p], half, n, znear, dtype)
        owns = covers & ((face[p] < 0) | (Z < depth[p]))
        grey = np.where((ix + iz) % 2 == 0, dtype(colors[0]), dtype(colors[1]))
        face[p][owns] = -1
        depth[p][owns] = Z[owns]
        tiles[p][owns] = (ix * n + iz)[owns]
        color[p][owns] = grey[owns][:, None]
        image[p][owns] = np.round(255 * grey[owns]).astype(np.uint8)[:, None]
    return dict(image=image, color=color, face=face, ground=tiles, depth=depth, ground_y=ground_y, screen=out['screen'])


def pixel_class(face, ground):
    """what a pixel shows as one integer: the face id, or -2 - tile on the plane, or -1 on the background"""
    return np.where(ground >= 0, -2 - ground.astype(np.int64), face.astype(np.int64))


TILT = MR.rotation((1.0, 0.1, 0.05), -12.0)         # a camera_rotation that pitches the camera down (and rolls it a little): the floor is not level on screen


def ellipsoid_scene(H, W, rings=20, segments=24):
    """``MR.three_person_scene`` on a coarser sphere (2 + rings * segments vertices): the same half axes, tilts, translations and pseudo-focal length"""
    v, f = MR.uv_sphere(rings, segments)
    big = MR.three_person_scene(H, W)
    tilts = [MR.rotation((0.3, 0.1, 1.0), 7.3), MR.rotation((1.0, 0.4, -0.2), -11.9), MR.rotation((0.2, 1.0, 0.5), 23.1)]
    verts = np.stack([(v * np.array([0.25, 0.70, 0.20])) @ R.T for R in tilts]).astype(np.float32)
    return verts, f, big[2], big[3]


SCENES = [(size, angle, tilted) for size in ((96, 128), (180, 240)) for angle in (0, 270) for tilted in (False, True)]
_cache = {}


def scene_reference(size, angle, tilted):
    """the float64 picture of a scene of SCENES, computed once per session and shared (callers leave it unchanged) -> (scene, reference dict)"""
    key = (size, angle, tilted)
    if key not in _cache:
        H, W = size
        verts, faces, cam_t, focal = ellipsoid_scene(H, W)
        rot = TILT if tilted else None
        ref = render(np.zeros((H, W, 3), np.uint8), verts, faces, cam_t, focal, rot=rot, sideview_angle=angle)
        _cache[key] = (dict(verts=verts, faces=faces, cam_t=cam_t, focal=focal, rot=rot), ref)
    return _cache[key]
