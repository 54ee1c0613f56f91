"""float64 numpy restatement of the marked form of the mesh renderer (whmr_mesh_render_marked: keypoint skeletons and hidden-line wireframe), written
from the definition in docs/kernels.md, not from the kernel.  Built on tests/mesh_render_reference.py for everything that concerns the mesh (camera,
coverage, winner, shading).  Test infrastructure: the package never imports it.

Pixel (j, i) has the centre c = (i + 0.5, j + 0.5).  A bone (n0, n1) with both w > 0 covers c by a = clamp(half_width + 0.5 - d, 0, 1), d the distance
from c to the segment; a joint with w > 0 by a = clamp(radius + 0.5 - |c - k|, 0, 1); each with a > 0 blends C <- C + a (rgb - C), the skeletons of a
layer in table order, bones before joints.  A wireframe draw's winning face has alpha = clamp(half_width + 0.5 - d_e, 0, 1), d_e the distance to the
nearest of its three edge lines."""
import numpy as np

import mesh_ground_reference as MG
import mesh_render_reference as MR


def keypoints(joints, cam_t, focal, center, rot=None, sideview_angle=0, znear=MR.ZNEAR, dtype=np.float64):
    """source 0: joints [J, 3] (mesh frame) of one row -> (u, v, w) [J, 3]; w = the depth Z if u, v, Z are finite and Z > znear, else 0"""
    with np.errstate(all='ignore'):
        s = MR.project(np.asarray(joints, dtype)[None], np.asarray(cam_t, dtype).reshape(1, 3), np.asarray(focal, dtype).reshape(1, 2), center, rot,
                       sideview_angle, dtype)[0]
        ok = np.isfinite(s).all(1) & (s[:, 2] > znear)
    return np.concatenate([s[:, :2], np.where(ok, s[:, 2], 0)[:, None]], 1)


def given_keypoints(kp, dtype=np.float64):
    """source 1: (x, y, conf) [J, 3] -> (x, y, w), w = conf, or 0 if one of the three is not finite"""
    kp = np.asarray(kp, dtype)
    return np.concatenate([kp[:, :2], np.where(np.isfinite(kp).all(1), kp[:, 2], 0)[:, None]], 1)


def cover(H, W, a, b, reach, dtype=np.float64):
    """coverage [H, W] of every pixel centre by the segment a -> b (a == b: a dot)"""
    px = (np.arange(W, dtype=dtype) + 0.5)[None, :] * np.ones((H, 1), dtype)
    py = (np.arange(H, dtype=dtype) + 0.5)[:, None] * np.ones((1, W), dtype)
    d = np.asarray(b, dtype) - np.asarray(a, dtype)
    len2 = d @ d
    t = np.zeros((H, W), dtype)
    if len2 > 0:
        t = np.clip(((px - a[0]) * d[0] + (py - a[1]) * d[1]) / len2, 0, 1)
    dist = np.hypot(px - (a[0] + t * d[0]), py - (a[1] + t * d[1]))
    return np.clip(dtype(reach) - dist, 0, 1)


def layer(C, skeletons, bones, bone_rgb, joint_rgb, dtype=np.float64):
    """the skeletons (kp [J, 3], half_width, radius) in order over the colour C [H, W, 3], in place -> the pixels a mark touched [H, W]"""
    H, W = C.shape[:2]
    touched = np.zeros((H, W), bool)
    for kp, half_width, radius in skeletons:
        J = kp.shape[0]
        marks = []
        for e, (n0, n1) in enumerate(np.asarray(bones).reshape(-1, 2).tolist()):
            if 0 <= n0 < J and 0 <= n1 < J and kp[n0, 2] > 0 and kp[n1, 2] > 0:
                marks.append((kp[n0, :2], kp[n1, :2], half_width + 0.5, bone_rgb[e]))
        marks += [(kp[j, :2], kp[j, :2], radius + 0.5, joint_rgb[j]) for j in range(J) if kp[j, 2] > 0]
        for a, b, reach, rgb in marks:
            cov = cover(H, W, a, b, reach, dtype)
            on = cov > 0
            C[on] += cov[on][:, None] * (np.asarray(rgb, dtype)[None] - C[on])
            touched |= on
    return touched


def wire_alpha(fid, scr, faces, half_width, dtype=np.float64):
    """alpha [H, W] of a wireframe draw's pixels: fid [H, W] the winning face of THIS draw's faces or -1 (alpha 0 there), scr [V, 3] its screen vertices"""
    H, W = fid.shape
    f = np.where(fid >= 0, fid, 0)
    tri = scr[faces[f]][..., :2]                                                # [H, W, 3, 2]
    px = (np.arange(W, dtype=dtype) + 0.5)[None, :] * np.ones((H, 1), dtype)
    py = (np.arange(H, dtype=dtype) + 0.5)[:, None] * np.ones((1, W), dtype)
    d = np.full((H, W), np.inf, dtype)
    with np.errstate(all='ignore'):
        for k in range(3):
            a, b = tri[:, :, (k + 1) % 3], tri[:, :, (k + 2) % 3]
            e = (px - a[..., 0]) * (b[..., 1] - a[..., 1]) - (py - a[..., 1]) * (b[..., 0] - a[..., 0])
            d = np.fmin(d, np.abs(e) / np.hypot(b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]))
    return np.where(fid >= 0, np.clip(dtype(half_width) + 0.5 - d, 0, 1), 0)


def render_image(frame, size, center, rot, draws, skeletons, faces, bones, bone_rgb, joint_rgb, base=(0.65, 0.74, 0.86), znear=MR.ZNEAR, dtype=np.float64):
    """One target image.  frame uint8 [H, W, 3] or None (black); draws: (global draw index, verts [V, 3], cam_t [3], focal [2], sideview_angle, mode,
    half_width) per draw of this image in table order; skeletons: (kp [J, 3] = (u, v, w), layer, half_width, radius) of this image in table order.
    Returns dict(image uint8, overlay, color, face (draw * F + face or -1), depth, alpha, touched (by a mark), under, over)."""
    H, W = size
    F = faces.shape[0]
    face = np.full((H, W), -1, np.int64)
    depth, col, alpha = np.zeros((H, W), dtype), np.zeros((H, W, 3), dtype), np.zeros((H, W), dtype)
    if draws:
        scr = np.stack([MR.project(np.asarray(v, dtype)[None], np.asarray(t, dtype).reshape(1, 3), np.asarray(f, dtype).reshape(1, 2), center, rot, ang, dtype)[0]
                        for _, v, t, f, ang, _, _ in draws])
        nrm = np.stack([MR.vertex_normals(np.asarray(v, dtype)[None], faces, ang, dtype)[0] for _, v, _, _, ang, _, _ in draws])
        fid, dep, bary = MR.rasterize(scr, faces, H, W, False, znear, dtype)
        col = MR.shade(fid, bary, nrm, faces, base, dtype=dtype)[0]
        fid, depth = fid[0].astype(np.int64), dep[0]
        local = np.where(fid >= 0, fid // F, -1)
        alpha = (fid >= 0).astype(dtype)
        for k, (gid, _, _, _, _, mode, half_width) in enumerate(draws):
            mine = local == k
            face[mine] = gid * F + fid[mine] % F
            if mode == 1:
                alpha[mine] = wire_alpha(np.where(mine, fid % F, -1), scr[k], faces, half_width, dtype)[mine]
    C = np.zeros((H, W, 3), dtype) if frame is None else frame.astype(dtype) / 255
    under = layer(C, [(kp, hw, r) for kp, lay, hw, r in skeletons if lay == 0], bones, bone_rgb, joint_rgb, dtype)
    full, part = alpha == 1, (alpha > 0) & (alpha < 1)
    C[full] = col[full]
    C[part] += alpha[part][:, None] * (col[part] - C[part])
    over = layer(C, [(kp, hw, r) for kp, lay, hw, r in skeletons if lay == 1], bones, bone_rgb, joint_rgb, dtype)
    back = np.zeros((H, W, 3), np.uint8) if frame is None else frame
    image = np.round(255 * C).astype(np.uint8)
    untouched = ~under & ~over & (alpha == 0)
    image[untouched] = back[untouched]
    today = full & ~over
    image[today] = np.round(255 * col[today]).astype(np.uint8)
    return dict(image=image, overlay=C, color=col, face=face, depth=depth, alpha=alpha, touched=under | over, under=under, over=over)


def synthetic_joints(rng, n=49, radii=(0.25, 0.70, 0.20), scale=1.2):
    """n points uniform in the person's bounding ellipsoid scaled by 1.2 (mesh frame): some bones cross the silhouette, some leave a small image"""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * rng.uniform(size=(n, 1)) ** (1 / 3) * np.asarray(radii) * scale).astype(np.float32)


# ---- the scene of tests/test_mesh_marks_gpu.py: three images of three sizes in one call, four rows (the focal length belongs to the row)
SIZES = [(96, 128), (60, 80), (45, 67)]
SEED = 5
_cache = {}


def scene():
    verts, faces, cam_t, _ = MG.ellipsoid_scene(96, 128)
    rows = [0, 1, 1, 0]                                                           # person of every row
    image_of_row = [0, 0, 1, 2]
    focal = np.array([[np.hypot(*SIZES[i])] * 2 for i in image_of_row], np.float32)
    rng = np.random.default_rng(SEED)
    joints = np.stack([synthetic_joints(rng) for _ in rows])
    # (row, verts_set, image, angle): a wireframe and a solid draw share image 0; image 1 is a 270 degree side view in wireframe; image 2 is solid
    draws = [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 1, 270), (3, 0, 2, 0)]
    wire, width = [True, False, True, False], [1.0, 1.0, 1.6, 1.0]
    # (row, image, source, layer, angle, bone_width, joint_radius)
    skeletons = [(0, 0, 0, 'under', 0, 2.0, 2.0), (1, 0, 0, 'over', 0, 1.2, 1.5), (2, 1, 0, 'under', 270, 1.5, 1.0), (2, 1, 0, 'over', 270, 0.8, 2.5),
                 (3, 2, 0, 'over', 0, 1.0, 1.2)]
    frames = [np.random.default_rng(31 + i).integers(0, 256, size=hw + (3,), dtype=np.uint8) for i, hw in enumerate(SIZES)]
    cam_t = cam_t[rows].copy()
    cam_t[3] += np.array([-0.9, 0.35, 0.0], np.float32)                         # the person of image 2 stands half outside it: bones leave the image
    return dict(verts=verts[rows], faces=faces, cam_t=cam_t, focal=focal, joints=joints, draws=draws, wire=wire, width=width, skeletons=skeletons,
                frames=frames, sizes=SIZES)


def scene_reference(tilted, bones, bone_rgb, joint_rgb):
    """the float64 pictures of ``scene`` under the identity or the tilted camera, computed once per session and shared (callers leave them unchanged)
    -> (scene, [render_image dict per image], keypoints [S, J, 3])"""
    if tilted not in _cache:
        sc = scene()
        rot = MG.TILT if tilted else None
        kps, refs = [], []
        for row, img, _, _, ang, _, _ in sc['skeletons']:
            h, w = sc['sizes'][img]
            kps.append(keypoints(sc['joints'][row], sc['cam_t'][row], sc['focal'][row], (w // 2, h // 2), rot, ang))
        for i, (h, w) in enumerate(sc['sizes']):
            dr = [(d, sc['verts'][r], sc['cam_t'][r], sc['focal'][r], ang, int(sc['wire'][d]), 0.5 * sc['width'][d])
                  for d, (r, _, im, ang) in enumerate(sc['draws']) if im == i]
            sk = [(kps[s], 0 if lay == 'under' else 1, 0.5 * bw, jr) for s, (_, im, _, lay, _, bw, jr) in enumerate(sc['skeletons']) if im == i]
            refs.append(render_image(sc['frames'][i], (h, w), (w // 2, h // 2), rot, dr, sk, sc['faces'], bones, bone_rgb, joint_rgb))
        _cache[tilted] = (dict(sc, rot=rot), refs, np.stack(kps))
    return _cache[tilted]


def non_vacuous(sc, refs, kps):
    """marks touch > 2 % of the pixels, at least 50 mark pixels lie over mesh and 50 outside it, wire alpha is strictly between 0 and 1 on at least 50
    pixels, a skeleton has joints outside its image and both layers are used"""
    total = sum(h * w for h, w in sc['sizes'])
    touched = sum(x['touched'].sum() for x in refs)
    on_mesh = sum((x['touched'] & (x['face'] >= 0)).sum() for x in refs)
    partial = sum(((x['alpha'] > 0) & (x['alpha'] < 1)).sum() for x in refs)
    h, w = sc['sizes'][2]
    outside = ((kps[4][:, 0] < 0) | (kps[4][:, 0] > w) | (kps[4][:, 1] < 0) | (kps[4][:, 1] > h)).sum()
    return (touched > 0.02 * total and on_mesh >= 50 and touched - on_mesh >= 50 and partial >= 50 and outside >= 5
            and all(x['under'].any() or x['over'].any() for x in refs) and refs[0]['under'].any() and refs[0]['over'].any())
