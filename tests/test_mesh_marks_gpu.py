"""Keypoint skeletons and hidden-line wireframe of the mesh renderer on the device (whmr_mesh_render_marked: the ``wireframe`` / ``joints`` /
``keypoints_2d`` arguments of whmr_amd.utils.renderer_cam) against their float64 restatement (tests/mesh_marks_reference.py), and the marked form
against the entries it extends (torch.equal: same device code).  The bounds are those of tests/test_mesh_render_gpu.py."""
import numpy as np
import pytest
import torch

import mesh_ground_reference as MG
import mesh_marks_reference as MM
import mesh_render_reference as MR

pytestmark = pytest.mark.gpu

WANT = ('face', 'color', 'depth', 'ground', 'overlay', 'keypoints')


def _up(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _renderer(faces):
    from whmr_amd.utils.renderer_cam import MeshRenderer
    r = MeshRenderer(faces)
    return r, np.broadcast_to(r.joint_color, (49, 3))


def _draw(r, sizes, draws, frames, rows, wire=False, width=None, skeletons=(), joints=None, keypoints=None, rot=None, grounds=None, want=WANT,
          marked=True):
    """one call through the planners: -> (output images, result dict, pix_off per image)"""
    verts, cam_t, focal = rows
    outputs = [torch.zeros(tuple(hw) + (3,), dtype=torch.uint8, device=verts.device) for hw in sizes]
    images, table, total = r.plan_draws(sizes, draws, n_rows=verts.shape[0])
    g = None if grounds is None else r.plan_grounds(len(sizes), draws, grounds)
    extra = {}
    if marked:
        extra = dict(styles=r.plan_styles(len(draws), wire, width), skeletons=r.plan_skeletons(len(sizes), list(skeletons), n_rows=verts.shape[0]),
                     joints=joints, keypoints=keypoints)
    res = r._run_draws(images, table, total, frames, outputs, verts, None, cam_t, focal, rot, 0.05, want, grounds=g, **extra)
    return outputs, res, images['pix_off'].tolist()


def _compare(outputs, res, offs, sizes, refs, kps, what):
    """every image of one call against the restatement -> the measured figures.  The bounds of tests/test_mesh_render_gpu.py: the class of a pixel
    (face id or background) differs on < 2e-3 of the pixels; on agreeing pixels 'overlay' max error < 1e-3, median < 1e-6 and the bytes within one
    grey level; 'keypoints' < 1e-4 (u, v where the joint is drawn, and w)."""
    differ, n, oerr, berr = 0, 0, [], 0
    for i, ((h, w), ref) in enumerate(zip(sizes, refs)):
        face = res['face'][offs[i]:offs[i] + h * w].view(h, w).cpu().numpy()
        agree = face == ref['face']
        differ, n = differ + (~agree).sum(), n + h * w
        over = res['overlay'][offs[i]:offs[i] + h * w].view(h, w, 3).cpu().numpy().astype(np.float64)
        oerr.append(np.abs(over - ref['overlay'])[agree].reshape(-1))
        berr = max(berr, int(np.abs(outputs[i].cpu().numpy().astype(np.int64) - ref['image'].astype(np.int64))[agree].max()))
    oerr = np.concatenate(oerr)
    kp = res['keypoints'].cpu().numpy().astype(np.float64)
    drawn = kps[..., 2] > 0
    assert np.array_equal(kp[..., 2] > 0, drawn)
    kerr = max(np.abs(kp[..., 2] - kps[..., 2]).max(), np.abs(kp[..., :2] - kps[..., :2])[drawn].max()) if drawn.any() else 0.0
    print('%s: class differs on %.2e of the pixels; overlay error max %.2e median %.2e; bytes differ by at most %d; keypoints %.2e'
          % (what, differ / n, oerr.max(), np.median(oerr), berr, kerr))
    assert differ / n < 2e-3
    assert oerr.max() < 1e-3 and np.median(oerr) < 1e-6
    assert berr <= 1
    assert kerr < 1e-4
    return differ / n, oerr.max(), np.median(oerr), berr, kerr


def _scene(dev, tilted):
    r, jr = _renderer(MG.ellipsoid_scene(96, 128)[1])
    sc, refs, kps = MM.scene_reference(tilted, r.bones, r.bone_colors, jr)
    assert MM.non_vacuous(sc, refs, kps)
    rows = _up(dev, sc['verts'], sc['cam_t'], sc['focal'])
    frames = _up(dev, *sc['frames'])
    joints, = _up(dev, sc['joints'])
    return r, sc, refs, kps, rows, frames, joints


@pytest.mark.parametrize('tilted', [False, True])
def test_against_the_float64_restatement(dev, tilted):
    """images of 96 x 128, 60 x 80 and 45 x 67 in ONE call (widths that are no multiple of 64: the 256-pixel spans of the resolve straddle rows),
    ellipsoid persons of 962 vertices, front view, a 270 degree side view, identity and tilted camera, a wireframe and a solid draw sharing image 0,
    skeletons of 49 synthetic joints under and over the meshes, one person half outside its image.
    Measured on the device: class differs on 0 of the pixels; overlay error max 5.8e-6 (identity) / 8.3e-6 (tilted), median 9.0e-9; bytes differ by
    at most 1 grey level; keypoints 6.1e-6 / 5.4e-6"""
    r, sc, refs, kps, rows, frames, joints = _scene(dev, tilted)
    outputs, res, offs = _draw(r, sc['sizes'], sc['draws'], frames, rows, sc['wire'], sc['width'], sc['skeletons'], joints=joints, rot=sc['rot'])
    _compare(outputs, res, offs, sc['sizes'], refs, kps, 'marks, tilted %s' % tilted)
    assert (res['ground'] == -1).all() and torch.isnan(res['ground_y']).all()


def test_exact_identities(dev):
    r, sc, refs, kps, rows, frames, joints = _scene(dev, False)
    sizes, draws, F = sc['sizes'], sc['draws'], sc['faces'].shape[0]
    grounds = [(1, 2, None), (2, 3, -0.6)]
    want = ('face', 'color', 'depth', 'ground')
    # no marks + all solid: the scene form's bytes and planes, ground planes included
    a, ra, _ = _draw(r, sizes, draws, frames, rows, grounds=grounds, want=want, marked=False)
    b, rb, offs = _draw(r, sizes, draws, frames, rows, grounds=grounds, want=want + ('overlay',))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(ra[k], rb[k]) for k in want) and torch.equal(ra['ground_y'][1:], rb['ground_y'][1:])
    assert (rb['ground'] >= 0).float().mean() > 0.05 and (rb['face'] >= 0).float().mean() > 0.05
    plain, rp, _ = _draw(r, sizes, draws, frames, rows, want=('face',), marked=False)
    # a line wider than any face: the solid call's bytes
    wide, _, _ = _draw(r, sizes, draws, frames, rows, wire=True, width=1e4, want=())
    assert all(torch.equal(x, y) for x, y in zip(wide, plain))
    # the full call: bytes == rint(255 overlay) wherever a mark or a partial alpha touched the pixel; two runs give the same bits
    full, rf, _ = _draw(r, sizes, draws, frames, rows, sc['wire'], sc['width'], sc['skeletons'], joints=joints)
    again, rg, _ = _draw(r, sizes, draws, frames, rows, sc['wire'], sc['width'], sc['skeletons'], joints=joints)
    assert all(torch.equal(x, y) for x, y in zip(full, again)) and all(torch.equal(rf[k], rg[k]) for k in WANT)
    for i, ((h, w), ref) in enumerate(zip(sizes, refs)):
        over = rf['overlay'][offs[i]:offs[i] + h * w].view(h, w, 3)
        touched = torch.from_numpy(ref['touched'] | ((ref['alpha'] > 0) & (ref['alpha'] < 1))).to(dev)
        assert touched.sum() > 100 and torch.equal(full[i][touched], torch.round(255 * over[touched]).to(torch.uint8))
        assert torch.equal(rf['face'][offs[i]:offs[i] + h * w], rp['face'][offs[i]:offs[i] + h * w])        # the winner is the winner, wireframe or not
    # an under-layer skeleton leaves every solid-mesh pixel as the plain call has it; an over-layer skeleton changes some of them
    under = [(row, img, 0, 'under', ang, 2.0, 2.0) for row, _, img, ang in draws]
    over = [(row, img, 0, 'over', ang, 2.0, 2.0) for row, _, img, ang in draws]
    u, ru, _ = _draw(r, sizes, draws, frames, rows, skeletons=under, joints=joints)
    o, ro, _ = _draw(r, sizes, draws, frames, rows, skeletons=over, joints=joints)
    changed = 0
    for i, (h, w) in enumerate(sizes):
        mesh = (rp['face'][offs[i]:offs[i] + h * w] >= 0).view(h, w)
        assert torch.equal(u[i][mesh], plain[i][mesh]) and not torch.equal(u[i][~mesh], plain[i][~mesh])
        changed += (o[i][mesh] != plain[i][mesh]).any(-1).sum().item()
    assert changed > 100
    # source 1 fed with the 'keypoints' of the source-0 call: identical bytes (the rows of the keypoints are the skeletons of that call)
    sk = sc['skeletons']
    assert torch.equal(rf['keypoints'][2], rf['keypoints'][3])                                              # skeletons 2 and 3 draw row 2
    given = torch.stack([rf['keypoints'][s] for s in (0, 1, 2, 4)]).contiguous()                            # rows 0, 1, 2, 3
    fed, rk, _ = _draw(r, sizes, draws, frames, rows, sc['wire'], sc['width'], [(row, img, 1, lay, ang, bw, jr) for row, img, _, lay, ang, bw, jr in sk],
                       keypoints=given)
    assert all(torch.equal(x, y) for x, y in zip(fed, full)) and torch.equal(rk['overlay'], rf['overlay']) and torch.equal(rk['keypoints'], rf['keypoints'])


def _one_person(dev, size=(48, 64)):
    h, w = size
    verts, faces, cam_t, _ = MG.ellipsoid_scene(96, 128)
    r, jr = _renderer(faces)
    focal = np.full((1, 2), np.hypot(h, w), np.float32)
    frame = np.random.default_rng(41).integers(0, 256, size=size + (3,), dtype=np.uint8)
    return r, jr, verts[1:2], faces, cam_t[1:2], focal, frame


def _reference_one(r, jr, size, verts, faces, cam_t, focal, frame, kps_of_skeletons, skeletons, draw=True, wire=False, width=1.0):
    h, w = size
    dr = [(0, verts[0], cam_t[0], focal[0], 0, int(wire), 0.5 * width)] if draw else []
    sk = [(kp, 0 if lay == 'under' else 1, 0.5 * bw, rad) for kp, (_, _, _, lay, _, bw, rad) in zip(kps_of_skeletons, skeletons)]
    return MM.render_image(frame, size, (w // 2, h // 2), None, dr, sk, faces, r.bones, r.bone_colors, jr)


def test_edges(dev):
    """a NaN joint, a joint behind znear, confidence <= 0, a zero-length bone, a bone wholly off-image, a bone index >= J (a skeleton table with 49
    joints drawn with 30 keypoints), S = 0 with D > 0 and D = 0 with S > 0: nothing faults, and every picture is the restatement's.
    Measured on the device: not recorded yet (the test prints the figures)"""
    size = (48, 64)
    r, jr, verts, faces, cam_t, focal, frame = _one_person(dev, size)
    rows = _up(dev, verts, cam_t, focal)
    fr, = _up(dev, frame)
    draws = [(0, 0, 0, 0)]
    rng = np.random.default_rng(SEED_EDGES)
    j3 = MM.synthetic_joints(rng)[None].copy()
    j3[0, 3] = np.nan                                                              # bones 2 and 3 lose an end
    j3[0, 9] = (0.0, 0.0, -float(cam_t[0, 2]) + 0.01)                              # depth 0.01 < znear: behind the near plane
    j3[0, 13] = j3[0, 12]                                                          # bone (12, 13) has no length
    j3[0, 5:8, 0] += np.float32(40.0)                                               # bones (5, 6), (6, 7) far off the image
    j3[0, 22] = (np.inf, 0.0, 0.0)
    sk3 = [(0, 0, 0, 'under', 0, 2.0, 1.5), (0, 0, 0, 'over', 0, 1.0, 2.5)]
    kp3 = MM.keypoints(j3[0], cam_t[0], focal[0], (32, 24))
    assert (kp3[[3, 9, 22], 2] == 0).all() and (kp3[[5, 6, 7], 0] > 200).all() and (kp3[:, 2] > 0).sum() == 46
    k2 = np.concatenate([rng.uniform(-8, 72, size=(49, 2)), rng.uniform(-0.5, 1.0, size=(49, 1))], 1).astype(np.float32)[None]
    k2[0, 4] = (np.nan, 10.0, 1.0)
    k2[0, 6, 2] = 0.0
    k2[0, 11] = (20.0, 20.0, np.inf)
    sk2 = [(0, 0, 1, 'over', 0, 1.5, 2.0)]
    kp2 = MM.given_keypoints(k2[0])
    assert (kp2[:, 2] <= 0).sum() > 10 and (kp2[:, 2] > 0).sum() > 20
    worst = np.zeros(5)
    # 3-D joints with every kind of invalid one, under and over a solid mesh
    ref = _reference_one(r, jr, size, verts, faces, cam_t, focal, frame, [kp3, kp3], sk3)
    out, res, offs = _draw(r, [size], draws, [fr], rows, skeletons=sk3, joints=_up(dev, j3)[0])
    worst = np.maximum(worst, _compare(out, res, offs, [size], [ref], np.stack([kp3, kp3]), 'invalid 3-D joints'))
    # 2-D keypoints with confidences <= 0 and non-finite entries over a wireframe mesh
    ref = _reference_one(r, jr, size, verts, faces, cam_t, focal, frame, [kp2], sk2, wire=True, width=1.2)
    out, res, offs = _draw(r, [size], draws, [fr], rows, wire=True, width=1.2, skeletons=sk2, keypoints=_up(dev, k2)[0])
    worst = np.maximum(worst, _compare(out, res, offs, [size], [ref], kp2[None], 'invalid 2-D keypoints'))
    # a bone index >= J: the 49-joint skeleton drawn with 30 keypoints
    ref = _reference_one(r, jr[:30], size, verts, faces, cam_t, focal, frame, [kp2[:30]], sk2)
    out, res, offs = _draw(r, [size], draws, [fr], rows, skeletons=sk2, keypoints=_up(dev, k2[:, :30])[0])
    assert res['keypoints'].shape == (1, 30, 3)
    worst = np.maximum(worst, _compare(out, res, offs, [size], [ref], kp2[None, :30], '30 keypoints under 49-joint bones'))
    # S = 0 with D > 0
    ref = _reference_one(r, jr, size, verts, faces, cam_t, focal, frame, [], [], wire=True, width=1.2)
    out, res, offs = _draw(r, [size], draws, [fr], rows, wire=True, width=1.2)
    assert res['keypoints'].shape[0] == 0
    worst = np.maximum(worst, _compare(out, res, offs, [size], [ref], np.zeros(tuple(res['keypoints'].shape)), 'no skeleton'))
    # D = 0 with S > 0: the skeleton over the bare frame
    ref = _reference_one(r, jr, size, verts, faces, cam_t, focal, frame, [kp2], sk2, draw=False)
    out, res, offs = _draw(r, [size], [], [fr], rows, skeletons=sk2, keypoints=_up(dev, k2)[0])
    assert (res['face'] == -1).all() and not torch.equal(out[0], fr) and torch.equal(out[0][~torch.from_numpy(ref['touched']).to(dev)], fr[~torch.from_numpy(ref['touched']).to(dev)])
    worst = np.maximum(worst, _compare(out, res, offs, [size], [ref], kp2[None], 'no draw'))
    torch.cuda.synchronize()
    print('edges, worst: class %.2e, overlay max %.2e median %.2e, bytes %d, keypoints %.2e' % tuple(worst))


SEED_EDGES = 43


def test_more_skeletons_than_a_workgroup_bins(dev):
    """MESH_BIN_SKELETONS + 1 skeletons on one 48 x 64 image (and one on a second image, between them in the table): the last one is drawn by the
    pixel-by-pixel path, after the binned ones, in both layers.
    Measured on the device: not recorded yet (the test prints the figures)"""
    from whmr_amd import _lib as L
    size = (48, 64)
    r, jr, verts, faces, cam_t, focal, frame = _one_person(dev, size)
    n = L.MESH_BIN_SKELETONS + 1
    rng = np.random.default_rng(47)
    kp = np.concatenate([rng.uniform(0, 64, size=(n + 1, 49, 1)), rng.uniform(0, 48, size=(n + 1, 49, 1)), rng.uniform(-0.2, 1.0, size=(n + 1, 49, 1))],
                        2).astype(np.float32)
    order = list(range(n + 1))
    sk = [(row, 1 if row == 5 else 0, 1, 'over' if row % 3 == 0 else 'under', 0, 0.8, 0.8) for row in order]           # row 5 goes to image 1
    assert sk[-1][1] == 0 and sum(s[1] == 0 for s in sk) == n
    kps = np.stack([MM.given_keypoints(k) for k in kp])
    frame2 = np.random.default_rng(48).integers(0, 256, size=size + (3,), dtype=np.uint8)
    R = n + 1
    rows = _up(dev, np.repeat(verts, R, 0), np.repeat(cam_t, R, 0), np.repeat(focal, R, 0))
    h, w = size
    refs = []
    for img, fr in enumerate((frame, frame2)):
        mine = [s for s in order if sk[s][1] == img]
        refs.append(MM.render_image(fr, size, (w // 2, h // 2), None, [(img, verts[0], cam_t[0], focal[0], 0, 0, 0.5)],
                                    [(kps[s], 0 if sk[s][3] == 'under' else 1, 0.4, 0.8) for s in mine], faces, r.bones, r.bone_colors, jr))
    out, res, offs = _draw(r, [size, size], [(0, 0, 0, 0), (1, 0, 1, 0)], _up(dev, frame, frame2), rows, skeletons=sk, keypoints=_up(dev, kp)[0])
    _compare(out, res, offs, [size, size], refs, kps, '%d skeletons on one image' % n)
    # the last skeleton alone changes the picture: it is not dropped
    less, _, _ = _draw(r, [size, size], [(0, 0, 0, 0), (1, 0, 1, 0)], _up(dev, frame, frame2), rows, skeletons=sk[:-1], keypoints=_up(dev, kp)[0], want=())
    assert not torch.equal(less[0], out[0]) and torch.equal(less[1], out[1])


def test_strips_and_clips(dev):
    """render_clip_groups(keypoints_2d=) is render_image_group per person bit for bit; panel 0 differs from the frame only where marks lie, panel 1
    carries the skeleton under its mesh, the side panels none; render_clip is render per frame"""
    from whmr_amd.utils.renderer_cam import render_clip_groups, render_image_group
    H, W = 96, 128
    local_np, faces, cam_t, focal = MG.ellipsoid_scene(H, W)
    r, jr = _renderer(faces)
    frames = torch.from_numpy(np.random.default_rng(22).integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)).to(dev)
    index = [0, 1, 1]
    local, dt, df = _up(dev, local_np, cam_t, focal)
    world = (local @ torch.from_numpy(MR.rotation((1.0, 0.0, 0.3), 20.0).astype(np.float32)).to(dev).T).contiguous()
    rng = np.random.default_rng(MM.SEED)
    joints, = _up(dev, np.stack([MM.synthetic_joints(rng) for _ in range(3)]))
    kp2 = r.render_clip(frames, local, dt, df, index, joints=joints, want=('keypoints',))['keypoints']             # their 2-D keypoints, (u, v, depth)
    plain = render_clip_groups(frames, dt, world, local, None, df, index, r)
    strips = render_clip_groups(frames, dt, world, local, None, df, index, r, keypoints_2d=kp2, wireframe=True)
    solid = render_clip_groups(frames, dt, world, local, None, df, index, r, keypoints_2d=kp2)
    for p, i in enumerate(index):
        fl = (float(focal[p]), float(focal[p]))
        one = render_image_group(frames[i], dt[p], world[p], local[p], None, fl, (W // 2, H // 2), r, keypoints_2d=kp2[p], wireframe=True)
        assert torch.equal(strips[p], one), p
        kps = kp2[p].cpu().numpy().astype(np.float64)
        ref0 = MM.render_image(frames[i].cpu().numpy(), (H, W), (W // 2, H // 2), None, [], [(kps, 0, 0.5 * 3.0, 3.0)], faces, r.bones, r.bone_colors, jr)
        untouched = torch.from_numpy(~ref0['touched']).to(dev)
        panel0 = solid[p][:, :W]
        assert torch.equal(panel0[untouched], frames[i][untouched]) and (panel0 != frames[i]).any(-1).sum() > 200
        assert np.abs(panel0.cpu().numpy().astype(np.int64) - ref0['image'].astype(np.int64)).max() <= 1
        # panel 1: the skeleton under the solid mesh is the render call's picture; the side panels are the plain strips'
        over = r.render(frames[i], local[p:p + 1], dt[p:p + 1], df[p:p + 1], keypoints_2d=kp2[p:p + 1])
        assert torch.equal(solid[p][:, W:2 * W], over) and not torch.equal(over, plain[p][:, W:2 * W])
        assert torch.equal(solid[p][:, 2 * W:], plain[p][:, 2 * W:])
        assert not torch.equal(strips[p][:, 2 * W:], plain[p][:, 2 * W:])                                          # wireframe reaches the side views
    # joints= in the strips: projected by the person's own camera, the same keypoints, the same strip
    by_joints = render_clip_groups(frames, dt, world, local, None, df, index, r, joints=joints)
    assert all(torch.equal(a, b) for a, b in zip(by_joints, solid))
    # render_clip against render per frame, all persons of a frame in one depth buffer
    clip = r.render_clip(frames, local, dt, df, index, joints=joints, wireframe=True, line_width=1.5, keypoints_layer='over', want=('overlay', 'keypoints'))
    for f in range(2):
        rows = [p for p, i in enumerate(index) if i == f]
        one = r.render(frames[f], local[rows], dt[rows], df[rows], joints=joints[rows], wireframe=True, line_width=1.5, keypoints_layer='over',
                       want=('overlay', 'keypoints'))
        assert torch.equal(clip['image'][f], one['image']) and torch.equal(clip['overlay'][f], one['overlay'])
        assert torch.equal(clip['keypoints'][rows], one['keypoints'])
        assert not torch.equal(one['image'], r.render(frames[f], local[rows], dt[rows], df[rows]))
    with pytest.raises(ValueError):
        r.render(frames[0], local, dt, df, joints=joints, keypoints_2d=kp2)
    with pytest.raises(ValueError):
        r.render(frames[0], local, dt, df, joints=joints[:2])


def test_capture_in_a_hip_graph_replays_the_eager_bits(dev):
    """fixed tables, one stream, no parallel branches: the joints are projected on the device, so new vertices and joints in the captured buffers
    give the eager picture of the new inputs"""
    r, sc, refs, kps, rows, frames, joints = _scene(dev, False)
    sizes, draws = sc['sizes'], sc['draws']
    verts, cam_t, focal = rows
    moved_verts = verts + torch.tensor([0.02, 0.11, 0.05], device=dev)
    moved_joints = joints + torch.tensor([-0.04, 0.06, 0.01], device=dev)
    eager = _draw(r, sizes, draws, frames, rows, sc['wire'], sc['width'], sc['skeletons'], joints=joints)
    moved = _draw(r, sizes, draws, frames, (moved_verts, cam_t, focal), sc['wire'], sc['width'], sc['skeletons'], joints=moved_joints)
    assert not torch.equal(eager[0][0], moved[0][0]) and not torch.equal(eager[1]['keypoints'], moved[1]['keypoints'])
    outputs = [torch.zeros(hw + (3,), dtype=torch.uint8, device=dev) for hw in sizes]
    images, table, total = r.plan_draws(sizes, draws, n_rows=4)
    tables = r.upload_draws(images, table, frames, outputs, dev, styles=r.plan_styles(4, sc['wire'], sc['width']),
                            skeletons=r.plan_skeletons(3, sc['skeletons'], n_rows=4))
    assert len(tables) == 5
    sv, sj = verts.clone(), joints.clone()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):
        r.run_draws(tables, 3, 4, total, sv, None, cam_t, focal, want=WANT, joints=sj)       # warm-up on the capture stream: tables and workspace exist
    torch.cuda.current_stream().wait_stream(cs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        cap = r.run_draws(tables, 3, 4, total, sv, None, cam_t, focal, want=WANT, joints=sj)
    for want_out, want_res, _ in (eager, moved):
        for o in outputs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outputs, want_out))
        assert all(torch.equal(cap[k], want_res[k]) for k in WANT)
        sv.copy_(moved_verts)
        sj.copy_(moved_joints)


def test_frame_pipeline_draws_wireframe_and_keypoints(dev, assets, state_dict):
    """FramePipeline(wireframe=True, draw_keypoints=True): another picture than the plain one, and its 'keypoints' are the package's own projection
    (demo.keypoints_full_image: SMPL.joints_from_vertices of local_smpl_vertices through whmr_perspective) -- two kernels evaluating
    cx + f (x + tx) / (z + tz) in fp32 at coordinates below 2^10, each within a few ulp (2^-14) of the exact value: they agree within 1e-3 pixels.
    Measured on the device: not recorded yet (the test prints the figures)"""
    from whmr_amd.demo import FramePipeline, keypoints_full_image
    from whmr_amd.models import whmr_net
    from whmr_amd.utils.renderer_cam import MeshRenderer
    _, faces = MR.uv_sphere()
    frame = torch.from_numpy(np.random.default_rng(3).integers(0, 256, size=(360, 640, 3), dtype=np.uint8)).to(dev)
    dets = [(320.0, 180.0, 220.0, 220.0), (100.5, 90.0, 150.0, 150.0)]
    m = whmr_net(None, assets=assets, numerics='bf16')
    m.load_state_dict(state_dict, strict=False)
    m = m.to(dev).eval()
    r = MeshRenderer(faces)
    out, plain = FramePipeline(m, renderer=r)(frame, dets)
    plain = plain.clone()
    out2, res = FramePipeline(m, renderer=r, wireframe=True, draw_keypoints=True, want=('keypoints',))(frame, dets)
    assert all(torch.equal(out[k], out2[k]) for k in out)
    assert res['image'].shape == plain.shape and not torch.equal(res['image'], plain)
    smpl = m.regressor[0].smpl
    joints = smpl.joints_from_vertices(out2['local_smpl_vertices'])
    assert joints.shape == (2, 49, 3)
    # the vertex joints are the vertices themselves; the regressed ones are the forward pass's regression of the same vertices
    ids = torch.tensor([s - 24 for s in smpl.joint_map.tolist() if 24 <= s < 45])
    picked = [j for j, s in enumerate(smpl.joint_map.tolist()) if 24 <= s < 45]
    assert torch.equal(joints[:, picked], out2['local_smpl_vertices'].float()[:, smpl.extra_joints_idxs[ids.to(dev)]])
    kp = keypoints_full_image(m, out2, (360, 640))
    assert kp.shape == (2, 49, 3) and (kp[..., 2] == 1).all()
    drawn = res['keypoints'][..., 2] > 0
    err = (res['keypoints'][..., :2] - kp[..., :2])[drawn].abs().max().item()
    print('pipeline keypoints: %d of 98 in front of the camera, renderer against keypoints_full_image %.2e pixels' % (drawn.sum().item(), err))
    assert drawn.sum() > 0 and err < 1e-3
    # fed back as 2-D keypoints they draw the same skeleton
    a = r.render(frame, out2['local_smpl_vertices'], out2['pred_cam_t'], out2['focal_length'], keypoints_2d=res['keypoints'], wireframe=True)
    assert torch.equal(a, res['image'])
