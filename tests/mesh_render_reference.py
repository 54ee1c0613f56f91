"""float64 numpy restatement of the mesh overlay renderer's contract (w-hmr_amd/csrc/mesh_render.hip), written from the contract and the reference call
sites (utils/renderer_cam.py:41-141, demo/tester.py:176-214), not from the kernel: camera, top-left coverage, nearest face with the global-face-id
tie-break, area-weighted smooth normals, the diffuse shading model and the uint8 rounding.  Test infrastructure: the package never imports it.
``dtype=np.float32`` runs the same arithmetic in single precision (how much of a difference to the device is rounding alone).

Also the test mesh: a UV sphere of 82 rings x 84 segments + two poles = 6890 vertices, 13776 faces -- SMPL's counts -- closed and wound outwards."""
import math

import numpy as np

AMBIENT = 0.3
K_D = 4 * (1 - 0.2) * (1 - 0.04) / math.pi          # n_lights (1 - metallic) (1 - 0.04) / pi
LIGHT = (0.0, 0.0, 1.0)                             # direction TO the light, world frame: every light shines along -z
ZNEAR = 0.05


def uv_sphere(rings=82, segments=84):
    """unit sphere, poles on the y axis: vertices [2 + rings * segments, 3] float64, faces [2 * segments * rings, 3] int32, outward winding"""
    th = np.pi * np.arange(1, rings + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.cos(th)[:, None] * np.ones_like(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None]], -1)
    v = np.concatenate([[[0.0, 1.0, 0.0]], ring.reshape(-1, 3), [[0.0, -1.0, 0.0]]])
    idx = lambda r, s: 1 + r * segments + (s % segments)
    faces = []
    for s in range(segments):
        faces.append((0, idx(0, s + 1), idx(0, s)))
        faces.append((len(v) - 1, idx(rings - 1, s), idx(rings - 1, s + 1)))
    for r in range(rings - 1):
        for s in range(segments):
            a, b, c, d = idx(r, s), idx(r, s + 1), idx(r + 1, s), idx(r + 1, s + 1)
            faces.append((a, b, c))
            faces.append((b, d, c))
    f = np.asarray(faces, dtype=np.int32)
    # outward: positive signed volume
    vol = np.einsum('ij,ij->i', v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum()
    if vol < 0:
        f = f[:, ::-1].copy()
    return v, f


def rot_y(deg, dtype=np.float64):
    a = math.radians(deg)
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], dtype=dtype)


def world_matrix(sideview_angle, dtype=np.float64):
    """mesh frame -> pyrender world: 180 degrees about X, then sideview_angle about Y (renderer_cam.py:75-82)"""
    return rot_y(sideview_angle, dtype) @ np.diag([1.0, -1.0, -1.0]).astype(dtype)


def project(verts, cam_t, focal, center, rot=None, sideview_angle=0, dtype=np.float64):
    """verts [P, V, 3], cam_t [P, 3], focal [P, 2] -> screen [P, V, 3] = (u, v, depth).  Scene of renderer_cam.py:71-114: t' = (-tx, ty, tz), camera
    pose [R | R t'], the camera looks down -z with y up: p_c = R^T q - t', u = cx + fx x_c / (-z_c), v = cy - fy y_c / (-z_c), depth -z_c."""
    verts, cam_t, focal = np.asarray(verts, dtype), np.asarray(cam_t, dtype), np.asarray(focal, dtype)
    R = np.eye(3, dtype=dtype) if rot is None else np.asarray(rot, dtype)
    q = verts @ world_matrix(sideview_angle, dtype).T
    tp = cam_t * np.array([-1.0, 1.0, 1.0], dtype)
    pc = q @ R - tp[:, None, :]                               # rows: R^T q
    depth = -pc[..., 2]
    u = dtype(center[0]) + focal[:, None, 0] * pc[..., 0] / depth
    v = dtype(center[1]) - focal[:, None, 1] * pc[..., 1] / depth
    return np.stack([u, v, depth], -1).astype(dtype)


def vertex_normals(verts, faces, sideview_angle=0, dtype=np.float64):
    """area-weighted smooth normals in the world frame: sum of (v1 - v0) x (v2 - v0) over the faces around a vertex, normalised"""
    verts = np.asarray(verts, dtype)
    n = np.zeros_like(verts)
    fn = np.cross(verts[:, faces[:, 1]] - verts[:, faces[:, 0]], verts[:, faces[:, 2]] - verts[:, faces[:, 0]])
    for p in range(verts.shape[0]):
        for k in range(3):
            np.add.at(n[p], faces[:, k], fn[p])
    n /= np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-30)
    return (n @ world_matrix(sideview_angle, dtype).T).astype(dtype)


def _edge(ax, ay, bx, by, px, py):
    """edge function of a -> b at p, evaluated from the lexicographically smaller end point and negated for the other direction: the two faces of a
    shared edge get the same number with opposite signs"""
    if bx < ax or (bx == ax and by < ay):
        return -((px - bx) * (ay - by) - (py - by) * (ax - bx))
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _top_left(ax, ay, bx, by):
    """for a face whose area (by _edge) is positive: a -> b is a left edge (interior towards +x) or a horizontal top edge (interior towards +y)"""
    return by > ay or (by == ay and bx < ax)


def rasterize(scr, faces, H, W, per_person=False, znear=ZNEAR, dtype=np.float64):
    """scr [P, V, 3] -> (face id [NI, H, W] int32 (person * F + face, -1 = background), depth [NI, H, W], bary [NI, H, W, 3] perspective-correct).
    Pixel (j, i) samples (i + 0.5, j + 0.5); top-left fill rule; nearest face wins, ties go to the smaller global id (faces are visited in
    increasing id and replace only on strictly smaller depth)."""
    scr = np.asarray(scr, dtype)
    P, F = scr.shape[0], faces.shape[0]
    NI = P if per_person else 1
    fid = np.full((NI, H, W), -1, np.int32)
    zb = np.full((NI, H, W), np.inf, dtype)
    bary = np.zeros((NI, H, W, 3), dtype)
    half = dtype(0.5)
    for p in range(P):
        img = p if per_person else 0
        tri = scr[p][faces]                                                   # [F, 3, 3]
        with np.errstate(invalid='ignore'):
            good = np.isfinite(tri[..., :2]).all((1, 2)) & (tri[..., 2] > znear).all(1)
        lo, hi = tri[..., :2].min(1), tri[..., :2].max(1)
        with np.errstate(invalid='ignore'):
            good &= (hi[:, 0] >= 0.5) & (hi[:, 1] >= 0.5) & (lo[:, 0] <= W - 0.5) & (lo[:, 1] <= H - 0.5)
        for f in np.nonzero(good)[0]:
            (ax, ay, az), (bx, by, bz), (cx, cy, cz) = tri[f]
            x0, x1 = max(int(math.ceil(lo[f, 0] - 0.5)), 0), min(int(math.floor(hi[f, 0] - 0.5)), W - 1)
            y0, y1 = max(int(math.ceil(lo[f, 1] - 0.5)), 0), min(int(math.floor(hi[f, 1] - 0.5)), H - 1)
            if x1 < x0 or y1 < y0:
                continue
            area = _edge(ax, ay, bx, by, cx, cy)
            if not (area != 0):
                continue
            px = (np.arange(x0, x1 + 1, dtype=dtype) + half)[None, :]
            py = (np.arange(y0, y1 + 1, dtype=dtype) + half)[:, None]
            with np.errstate(over='ignore', invalid='ignore'):
                e0, e1, e2 = _edge(bx, by, cx, cy, px, py), _edge(cx, cy, ax, ay, px, py), _edge(ax, ay, bx, by, px, py)
            sgn = dtype(1.0) if area > 0 else dtype(-1.0)
            if area > 0:
                t0, t1, t2 = _top_left(bx, by, cx, cy), _top_left(cx, cy, ax, ay), _top_left(ax, ay, bx, by)
            else:
                t0, t1, t2 = _top_left(cx, cy, bx, by), _top_left(ax, ay, cx, cy), _top_left(bx, by, ax, ay)
            s0, s1, s2 = sgn * e0, sgn * e1, sgn * e2
            inside = ((s0 > 0) | ((s0 == 0) & t0)) & ((s1 > 0) | ((s1 == 0) & t1)) & ((s2 > 0) | ((s2 == 0) & t2))
            if not inside.any():
                continue
            q0, q1, q2 = e0 / area / az, e1 / area / bz, e2 / area / cz
            with np.errstate(divide='ignore', invalid='ignore'):
                den = q0 + q1 + q2
                b0, b1, b2 = q0 / den, q1 / den, q2 / den
                pz = b0 * az + b1 * bz + b2 * cz
            zs = zb[img, y0:y1 + 1, x0:x1 + 1]
            win = inside & (pz > 0) & (pz < zs)
            if not win.any():
                continue
            zs[win] = pz[win]
            fid[img, y0:y1 + 1, x0:x1 + 1][win] = p * F + f
            bary[img, y0:y1 + 1, x0:x1 + 1][win] = np.stack([b0, b1, b2], -1)[win]
    zb[fid < 0] = 0
    return fid, zb, bary


def shade(fid, bary, normals, faces, base, ambient=AMBIENT, k_d=K_D, light=LIGHT, dtype=np.float64):
    """colour [NI, H, W, 3] in 0..1 (0 on the background): clamp(base (ambient + k_d max(n . l, 0)), 0, 1), n = the renormalised
    perspective-correct interpolation of the vertex normals"""
    F = faces.shape[0]
    cov = fid >= 0
    g = np.where(cov, fid, 0)
    p, f = g // F, g % F
    n = np.zeros(fid.shape + (3,), dtype)
    for k in range(3):
        n += bary[..., k:k + 1] * normals[p, faces[f, k]]
    n /= np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-30)
    ndl = np.maximum(n @ np.asarray(light, dtype), 0)
    lum = dtype(ambient) + dtype(k_d) * ndl
    col = np.clip(lum[..., None] * np.asarray(base, dtype), 0, 1)
    return np.where(cov[..., None], col, 0).astype(dtype)


def render(frame, verts, faces, cam_t, focal, center=None, rot=None, sideview_angle=0, per_person=False, base=(0.65, 0.74, 0.86), znear=ZNEAR,
           dtype=np.float64):
    """the whole contract: dict(image uint8 [H, W, 3] or [P, H, W, 3], color, face, depth, screen); frame uint8 [H, W, 3]"""
    H, W = frame.shape[:2]
    P = np.asarray(verts).shape[0]
    focal = np.asarray(focal, dtype).reshape(P, -1)
    focal = np.broadcast_to(focal, (P, 2)) if focal.shape[1] == 1 else focal
    center = (W // 2, H // 2) if center is None else center
    scr = project(verts, cam_t, focal, center, rot, sideview_angle, dtype)
    fid, depth, bary = rasterize(scr, faces, H, W, per_person, znear, dtype)
    col = shade(fid, bary, vertex_normals(verts, faces, sideview_angle, dtype), faces, base, dtype=dtype)
    img = np.where((fid >= 0)[..., None], np.round(255 * col).astype(np.uint8), frame[None])
    sq = (lambda a: a) if per_person else (lambda a: a[0])
    return dict(image=sq(img), color=sq(col), face=sq(fid), depth=sq(depth), screen=scr)


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(deg)
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * K @ K


def three_person_scene(H, W):
    """Three body-sized ellipsoids (half axes 0.25 x 0.70 x 0.20 m, each tilted a little so that no vertex row follows a pixel row) in front of the
    demo's pseudo-focal camera (focal = sqrt(H^2 + W^2), tester.py:134-136): persons 0 and 1 interpenetrate (0.35 m apart sideways, 0.15 m in depth),
    person 2 stands nearer and partly beyond the right border.  Returns float32 verts [3, 6890, 3], int32 faces, cam_t [3, 3], focal [3]."""
    v, f = uv_sphere()
    radii = np.array([0.25, 0.70, 0.20])
    tilts = [rotation((0.3, 0.1, 1.0), 7.3), rotation((1.0, 0.4, -0.2), -11.9), rotation((0.2, 1.0, 0.5), 23.1)]
    verts = np.stack([(v * radii) @ R.T for R in tilts]).astype(np.float32)
    cam_t = np.array([[-0.30, 0.05, 3.20], [0.05, -0.02, 3.35], [1.05, 0.21, 2.60]], np.float32)
    focal = np.full(3, math.sqrt(H * H + W * W), np.float32)
    return verts, f, cam_t, focal
