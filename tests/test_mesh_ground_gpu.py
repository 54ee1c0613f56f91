"""The checkerboard ground plane of the mesh renderer on the device (whmr_mesh_render_scene: the ``ground`` arguments of whmr_amd.utils.renderer_cam)
against its float64 restatement (tests/mesh_ground_reference.py), and the scene form against the draw list it extends (torch.equal: same device code)."""
import math

import numpy as np
import pytest
import torch

import mesh_ground_reference as MG
import mesh_render_reference as MR

pytestmark = pytest.mark.gpu

WANT = ('face', 'color', 'depth', 'ground')
DARK8, LIGHT8 = 35, 220                                       # rint(255 * 35 / 255), rint(255 * 220 / 255)


def _up(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _compare(out, ref, verts, what):
    """one call of per-person images with planes against the restatement: the bounds of tests/test_mesh_render_gpu.py (class of a pixel -- face id,
    tile or background -- differs on < 2e-3 of the pixels; colour on agreeing mesh pixels max < 1e-3, median < 1e-6; depth < 1e-4), the plane's
    bytes exactly, and the height bit for bit.  Measured on the device over all callers: class differs on 0 of the pixels, colour max 1.8e-5, median
    6.5e-8, depth 5.7e-6 on the mesh and 9.1e-7 on the plane"""
    face, tile, col, dep, img = (out[k].cpu().numpy() for k in ('face', 'ground', 'color', 'depth', 'image'))
    mine, want = MG.pixel_class(face, tile), MG.pixel_class(ref['face'], ref['ground'])
    differ = (mine != want).mean()
    mesh, plane = (mine == want) & (face >= 0), (mine == want) & (tile >= 0)
    cerr = np.abs(col.astype(np.float64) - ref['color'])[mesh]
    derr_mesh, derr_plane = np.abs(dep - ref['depth'])[mesh].max(), np.abs(dep - ref['depth'])[plane].max()
    print('%s: mesh on %.3f, plane on %.3f of the pixels; class differs on %.2e; colour error max %.2e median %.2e; depth error mesh %.2e plane %.2e'
          % (what, (ref['face'] >= 0).mean(), (ref['ground'] >= 0).mean(), differ, cerr.max(), np.median(cerr), derr_mesh, derr_plane))
    assert ((ref['face'] >= 0) | (ref['ground'] >= 0)).mean() > 0.02 and (ref['ground'] >= 0).mean() > 0.1       # a plane is in view
    assert differ < 2e-3
    assert cerr.max() < 1e-3 and np.median(cerr) < 1e-6
    assert derr_mesh < 1e-4 and derr_plane < 1e-4
    # plane pixels: face -1, the tile's grey exactly, in the fp32 colour and in the bytes
    on = tile >= 0
    light = ((tile // MG.TILES + tile % MG.TILES) % 2 == 1)
    assert (face[on] == -1).all() and tile.max() < MG.TILES ** 2
    assert np.array_equal(img[on], np.repeat(np.where(light[on], LIGHT8, DARK8).astype(np.uint8)[:, None], 3, 1))
    assert np.array_equal(col[on], np.repeat(np.where(light[on], np.float32(MG.LIGHT), np.float32(MG.DARK))[:, None], 3, 1))
    assert (on & light).any() and (on & ~light).any()
    # background: black, nothing in the planes
    bg = (face < 0) & ~on
    assert not img[bg].any() and not dep[bg].any() and not col[bg].any()
    # the height: -max p_y of the float32 vertices, bit for bit
    assert torch.equal(out['ground_y'].cpu(), -torch.from_numpy(verts)[:, :, 1].max(dim=1).values)
    assert np.array_equal(out['ground_y'].cpu().numpy().astype(np.float64), ref['ground_y'])


@pytest.mark.parametrize('size,angle,tilted', MG.SCENES)
def test_planes_against_the_float64_reference(dev, size, angle, tilted):
    """three ellipsoid persons (962 vertices: not a multiple of 64, waves of the height reduction straddle two persons), one image and one plane each,
    front and side view, level and pitched camera"""
    from whmr_amd.utils.renderer_cam import MeshRenderer
    scene, ref = MG.scene_reference(size, angle, tilted)
    r = MeshRenderer(scene['faces'])
    dv, dt, df = _up(dev, scene['verts'], scene['cam_t'], scene['focal'])
    out = r.render(None, dv, dt, df, size=size, rot=scene['rot'], sideview_angle=angle, per_person=True, ground=True, want=WANT)
    assert out['image'].shape == (3,) + size + (3,) and out['ground'].shape == (3,) + size and out['ground_y'].shape == (3,)
    _compare(out, ref, scene['verts'], '%dx%d angle %d tilted %s' % (size + (angle, tilted)))
    # without the plane: today's picture, and the plane took nothing from the mesh that the depth test did not give it
    bare = r.render(None, dv, dt, df, size=size, rot=scene['rot'], sideview_angle=angle, per_person=True, want=('face', 'depth'))
    kept = out['face'] >= 0
    assert torch.equal(out['face'][kept], bare['face'][kept]) and torch.equal(out['depth'][kept], bare['depth'][kept])
    lost = (bare['face'] >= 0) & ~kept
    assert (out['ground'][lost] >= 0).all() and (out['depth'][lost] < bare['depth'][lost]).all()


def test_smpl_sized_persons(dev):
    """MR.three_person_scene itself: 6890 vertices and 13776 faces per person"""
    from whmr_amd.utils.renderer_cam import MeshRenderer
    H, W = 96, 128
    verts, faces, cam_t, focal = MR.three_person_scene(H, W)
    ref = MG.render(np.zeros((H, W, 3), np.uint8), verts, faces, cam_t, focal, sideview_angle=270)
    dv, dt, df = _up(dev, verts, cam_t, focal)
    out = MeshRenderer(faces).render(None, dv, dt, df, size=(H, W), sideview_angle=270, per_person=True, ground=True, want=WANT)
    _compare(out, ref, verts, 'SMPL-sized, 96x128 side view')


@pytest.mark.parametrize('tilted', [False, True])
def test_depth_test_both_ways(dev, tilted):
    """a given height h = 0 cuts the ellipsoid at the waist; the camera stands above the plane: the mesh below the waist is hidden by the plane, the
    mesh above it hides the plane behind"""
    from whmr_amd.utils.renderer_cam import MeshRenderer
    H, W = 96, 128
    verts, faces, _, focal = MG.ellipsoid_scene(H, W)
    verts, focal, cam_t = verts[:1], focal[:1], np.array([[0.1, 0.45, 3.0]], np.float32)
    rot = MG.TILT if tilted else None
    frame = np.zeros((H, W, 3), np.uint8)
    ref = MG.render(frame, verts, faces, cam_t, focal, rot=rot, ground=0.0)
    bare = MR.render(frame, verts, faces, cam_t, focal, rot=rot, per_person=True)
    covers = MG.plane(H, W, cam_t[0], (focal[0], focal[0]), (W // 2, H // 2), rot, 0.0)[0]
    assert ((bare['face'][0] >= 0) & (ref['ground'][0] >= 0)).sum() > 200 and ((ref['face'][0] >= 0) & covers).sum() > 200       # both ways, in the restatement
    dv, dt, df = _up(dev, verts, cam_t, focal)
    r = MeshRenderer(faces)
    out = r.render(None, dv, dt, df, size=(H, W), rot=rot, ground=0.0, want=WANT)                     # a single row: no per_person needed
    assert out['image'].shape == (H, W, 3) and out['ground_y'].tolist() == [0.0]
    face, tile = out['face'].cpu().numpy(), out['ground'].cpu().numpy()
    differ = (MG.pixel_class(face, tile) != MG.pixel_class(ref['face'][0], ref['ground'][0])).mean()
    print('depth test, tilted %s: class differs on %.2e of the pixels' % (tilted, differ))
    assert differ < 2e-3
    assert ((bare['face'][0] >= 0) & (tile >= 0)).sum() > 200 and ((face >= 0) & covers).sum() > 200
    agree = (tile >= 0) & (ref['ground'][0] == tile)
    assert np.abs(out['depth'].cpu().numpy() - ref['depth'][0])[agree].max() < 1e-4
    # render_overlay_image hands the argument on
    from whmr_amd.utils.renderer_cam import render_overlay_image
    one = render_overlay_image(torch.zeros(H, W, 3, dtype=torch.uint8, device=dev), dt[0], dv[0], rot, (float(focal[0]), float(focal[0])), (W // 2, H // 2), r,
                               add_ground_plane=0.0)
    assert torch.equal(one, out['image'])


def _three_images(dev):
    """three rows drawn into three images of different sizes: the table rows of one call"""
    sizes = [(96, 128), (60, 80), (48, 64)]
    verts, faces, cam_t, _ = MG.ellipsoid_scene(96, 128)
    focal = np.array([math.sqrt(h * h + w * w) for h, w in sizes], np.float32)
    draws = [(0, 0, 0, 0), (1, 0, 1, 270), (2, 0, 2, 0)]
    frames = [torch.from_numpy(np.random.default_rng(21 + i).integers(0, 256, size=hw + (3,), dtype=np.uint8)).to(dev) for i, hw in enumerate(sizes)]
    return sizes, faces, draws, frames, _up(dev, verts, cam_t, focal.reshape(3, 1).repeat(2, 1))


def _draw(r, sizes, draws, grounds, frames, rows, want=WANT):
    verts, cam_t, focal = rows
    outputs = [torch.zeros(hw + (3,), dtype=torch.uint8, device=verts.device) for hw in sizes]
    images, table, total = r.plan_draws(sizes, draws, n_rows=verts.shape[0])
    g = None if grounds is None else r.plan_grounds(len(sizes), draws, grounds)
    res = r._run_draws(images, table, total, frames, outputs, verts, None, cam_t, focal, None, 0.05, want, grounds=g)
    return outputs, res, images['pix_off'].tolist()


def test_one_call_three_images(dev):
    """an image with a plane from its mesh, one with a given height and one without, of three sizes, in one call: the planed ones equal single-image
    calls bit for bit (the packed planes start at pix_off; the plane is a per-image branch), the third the draw list's bytes"""
    from whmr_amd.utils.renderer_cam import MeshRenderer
    sizes, faces, draws, frames, rows = _three_images(dev)
    r = MeshRenderer(faces)
    outputs, res, offs = _draw(r, sizes, draws, [(0, 0, None), (1, 1, -0.6)], frames, rows)
    gy = res['ground_y'].cpu()
    assert gy[0] == -rows[0][0, :, 1].max().cpu() and gy[1] == np.float32(-0.6) and torch.isnan(gy[2])
    for i, (angle, ground) in enumerate(((0, True), (270, -0.6))):
        one = r.render(frames[i], rows[0][i:i + 1], rows[1][i:i + 1], rows[2][i:i + 1], sideview_angle=angle, ground=ground, want=WANT)
        h, w = sizes[i]
        assert torch.equal(outputs[i], one['image']), i
        assert (one['ground'] >= 0).float().mean() > 0.1 and (one['face'] >= 0).float().mean() > 0.02
        for k in WANT:
            got = res[k][offs[i]:offs[i] + h * w].view(one[k].shape)
            got = torch.where(got >= 0, got - i * faces.shape[0], got) if k == 'face' else got          # global id = draw * F + face
            assert torch.equal(got, one[k]), (i, k)
    # the image without a plane: the draw list's bytes
    alone, plain, _ = _draw(r, sizes[2:], [(2, 0, 0, 0)], None, frames[2:], rows, want=('face', 'color', 'depth'))
    h, w = sizes[2]
    assert torch.equal(outputs[2], alone[0]) and (res['ground'][offs[2]:] == -1).all()
    for k in ('color', 'depth'):
        assert torch.equal(res[k][offs[2]:], plain[k]), k
    assert torch.equal(torch.where(res['face'][offs[2]:] >= 0, res['face'][offs[2]:] - 2 * faces.shape[0], res['face'][offs[2]:]), plain['face'])
    # two runs: identical bits
    again, res2, _ = _draw(r, sizes, draws, [(0, 0, None), (1, 1, -0.6)], frames, rows)
    assert all(torch.equal(a, b) for a, b in zip(outputs, again)) and all(torch.equal(res[k], res2[k]) for k in WANT)
    assert torch.equal(res['ground_y'][:2], res2['ground_y'][:2])


def test_a_table_without_planes_gives_the_bytes_of_the_draw_list(dev):
    from whmr_amd.utils.renderer_cam import MeshRenderer
    sizes, faces, draws, frames, rows = _three_images(dev)
    r = MeshRenderer(faces)
    draws = draws + [(1, 0, 0, 90)]                                                     # image 0 shared by two draws
    want = ('face', 'color', 'depth', 'screen')
    a, ra, _ = _draw(r, sizes, draws, None, frames, rows, want=want)
    b, rb, _ = _draw(r, sizes, draws, [], frames, rows, want=want + ('ground',))
    assert 'ground_y' not in ra and torch.isnan(rb['ground_y']).all() and (rb['ground'] == -1).all()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(ra[k], rb[k]) for k in want)
    assert (ra['face'] >= 0).float().mean() > 0.02


def test_strips_with_ground(dev):
    """render_clip_groups(ground=True): one launch group for the clip; panels 0 and 1 untouched, the whole strip what render_image_group draws per
    person (the planes go through the row-strided panels), each side view's floor at its own mesh's lowest point"""
    from whmr_amd.utils.renderer_cam import MeshRenderer, render_clip_groups, render_image_group
    H, W = 96, 128
    local_np, faces, cam_t, focal = MG.ellipsoid_scene(H, W)
    r = MeshRenderer(faces)
    frames = torch.from_numpy(np.random.default_rng(22).integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)).to(dev)
    index = [0, 1, 1]
    local, dt, df = _up(dev, local_np, cam_t, focal)
    world = (local @ torch.from_numpy(MR.rotation((1.0, 0.0, 0.3), 20.0).astype(np.float32)).to(dev).T).contiguous()      # smpl_vertices: upright elsewhere
    plain = render_clip_groups(frames, dt, world, local, None, df, index, r)
    strips = render_clip_groups(frames, dt, world, local, None, df, index, r, ground=True)
    assert len(strips) == 3 and strips[1].data_ptr() - strips[0].data_ptr() == H * 4 * W * 3
    for p, i in enumerate(index):
        assert torch.equal(strips[p][:, :2 * W], plain[p][:, :2 * W]), p
        fl = (float(focal[p]), float(focal[p]))
        ref = render_image_group(frames[i], dt[p], world[p], local[p], None, fl, (W // 2, H // 2), r, ground=True)
        assert torch.equal(strips[p], ref), p
        side = [r.render(None, v[p:p + 1], dt[p:p + 1], df[p:p + 1], size=(H, W), sideview_angle=270, ground=True, want=('ground',)) for v in (local, world)]
        for k in (0, 1):
            panel = strips[p][:, (2 + k) * W:(3 + k) * W]
            assert torch.equal(panel, side[k]['image']) and (side[k]['ground'] >= 0).float().mean() > 0.1
            assert not torch.equal(panel, plain[p][:, (2 + k) * W:(3 + k) * W])
        assert side[0]['ground_y'].item() == -local[p, :, 1].max().item() and side[1]['ground_y'].item() == -world[p, :, 1].max().item()
        assert side[0]['ground_y'].item() != side[1]['ground_y'].item() and not torch.equal(side[0]['image'], side[1]['image'])
    # a fixed floor over the clip
    fixed = render_clip_groups(frames, dt, world, local, None, df, index, r, ground=-0.75)
    ref = render_image_group(frames[1], dt[2], world[2], local[2], None, (float(focal[2]),) * 2, (W // 2, H // 2), r, ground=-0.75)
    assert torch.equal(fixed[2], ref) and not torch.equal(fixed[2], strips[2])


def test_render_clip_per_person_with_ground(dev):
    from whmr_amd.utils.renderer_cam import MeshRenderer
    sizes, faces, _, frames, rows = _three_images(dev)
    r = MeshRenderer(faces)
    verts, cam_t, focal = rows
    out = r.render_clip(frames, verts, cam_t, focal, [2, 0, 0], per_person=True, ground=True, want=('ground',))
    assert [tuple(i.shape[:2]) for i in out['image']] == [sizes[2], sizes[0], sizes[0]] and out['ground_y'].shape == (3,)
    for p, i in enumerate([2, 0, 0]):
        one = r.render(frames[i], verts[p:p + 1], cam_t[p:p + 1], focal[p:p + 1], ground=True, want=('ground',))
        assert torch.equal(out['image'][p], one['image']) and torch.equal(out['ground'][p], one['ground']) and out['ground_y'][p] == one['ground_y'][0]
    with pytest.raises(ValueError, match='ground plane'):
        r.render_clip(frames, verts, cam_t, focal, [2, 0, 0], ground=True)


def test_capture_in_a_hip_graph_replays_the_eager_bits(dev):
    """fixed tables, one stream, no parallel branches: the height is found and used on the device, so new vertices in the captured buffers give the
    eager picture of the new vertices, floor included"""
    from whmr_amd.utils.renderer_cam import MeshRenderer
    sizes, faces, draws, frames, rows = _three_images(dev)
    r = MeshRenderer(faces)
    verts, cam_t, focal = rows
    grounds = [(0, 0, None), (1, 1, -0.6)]
    moved_verts = verts + torch.tensor([0.02, 0.11, 0.05], device=dev)
    eager = _draw(r, sizes, draws, grounds, frames, rows)
    moved = _draw(r, sizes, draws, grounds, frames, (moved_verts, cam_t, focal))
    assert eager[1]['ground_y'][0] != moved[1]['ground_y'][0] and not torch.equal(eager[0][0], moved[0][0])
    outputs = [torch.zeros(hw + (3,), dtype=torch.uint8, device=dev) for hw in sizes]
    images, table, total = r.plan_draws(sizes, draws, n_rows=3)
    tables = r.upload_draws(images, table, frames, outputs, dev, grounds=r.plan_grounds(3, draws, grounds))
    assert len(tables) == 3
    sv = verts.clone()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):
        r.run_draws(tables, 3, 3, total, sv, None, cam_t, focal, want=WANT)              # warm-up on the capture stream: tables and workspace exist
    torch.cuda.current_stream().wait_stream(cs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        cap = r.run_draws(tables, 3, 3, total, sv, None, cam_t, focal, want=WANT)
    for want_out, want_res, _ in (eager, moved):
        for o in outputs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outputs, want_out))
        assert all(torch.equal(cap[k], want_res[k]) for k in WANT) and torch.equal(cap['ground_y'][:2], want_res['ground_y'][:2])
        sv.copy_(moved_verts)


def test_a_mesh_without_a_finite_vertex_gets_no_plane(dev):
    from whmr_amd.utils.renderer_cam import MeshRenderer
    H, W = 96, 128
    verts, faces, cam_t, focal = MG.ellipsoid_scene(H, W)
    verts = verts[:2].copy()
    verts[1] = np.nan
    verts[0, 5] = np.nan                                                                # a NaN vertex among numbers is skipped
    frame = torch.from_numpy(np.random.default_rng(23).integers(0, 256, size=(H, W, 3), dtype=np.uint8)).to(dev)
    dv, dt, df = _up(dev, verts, cam_t[:2], focal[:2])
    out = MeshRenderer(faces).render(frame, dv, dt, df, per_person=True, ground=True, want=WANT)
    torch.cuda.synchronize()
    gy = out['ground_y'].cpu().numpy()
    assert gy[0] == -np.nanmax(verts[0, :, 1]) and np.isnan(gy[1])
    assert torch.equal(out['image'][1], frame) and (out['ground'][1] == -1).all() and (out['face'][1] == -1).all() and not out['depth'][1].any()
    assert (out['ground'][0] >= 0).float().mean() > 0.1 and (out['face'][0] >= 0).float().mean() > 0.02
