"""Draw-list form of the overlay renderer (whmr_mesh_render_draws: MeshRenderer.render_clip, render_clip_groups, ClipPipeline) against the per-frame
renderer ``MeshRenderer.render`` -- itself held to the float64 restatement by tests/test_mesh_render_gpu.py.  Both entry points run the same device
code per vertex, face and pixel, so every comparison here is torch.equal: no tolerance."""
import math

import numpy as np
import pytest
import torch

import mesh_render_reference as MR

pytestmark = pytest.mark.gpu

SPHERE, FACES = MR.uv_sphere(rings=6, segments=7)            # 44 vertices, 84 faces: not a multiple of 64, waves of the face pass straddle two draws
NF = FACES.shape[0]


def _person(tilt):
    """a body-sized ellipsoid (half axes 0.25 x 0.70 x 0.20 m), tilted a little so that no vertex row follows a pixel row"""
    return (SPHERE * np.array([0.25, 0.70, 0.20])) @ MR.rotation((0.3, 0.2, 1.0), tilt).T


def _rows(dev, cam_t, sizes_of_rows):
    """verts [P, 44, 3], cam_t [P, 3], focal [P] (the pseudo-focal sqrt(H^2 + W^2) of each row's frame) on the device"""
    verts = np.stack([_person(7.0 + 5.0 * p) for p in range(len(cam_t))]).astype(np.float32)
    focal = np.array([math.sqrt(h * h + w * w) for h, w in sizes_of_rows], dtype=np.float32)
    return torch.from_numpy(verts).to(dev), torch.tensor(cam_t, dtype=torch.float32, device=dev), torch.from_numpy(focal).to(dev)


def _frames(dev, sizes, seed, strided=()):
    rng = np.random.default_rng(seed)
    out = []
    for i, (h, w) in enumerate(sizes):
        pad = 13 if i in strided else 0                        # a non-contiguous view: rows of a wider image
        out.append(torch.from_numpy(rng.integers(0, 256, size=(h, w + pad, 3), dtype=np.uint8)).to(dev)[:, :w])
    return out


@pytest.fixture(scope='module')
def scene(dev):
    """three frames of different sizes with [2, 0, 2] rows: the persons of frame 0 interpenetrate; in frame 2 one stands partly beyond the right border
    and one has its nearest vertices behind znear.  The per-frame pictures of ``render`` are computed once and left unchanged."""
    from whmr_amd.utils.renderer_cam import MeshRenderer
    sizes = [(48, 64), (40, 56), (33, 47)]
    index = [0, 0, 2, 2]
    frames = _frames(dev, sizes, 11, strided=(2,))
    assert not frames[2].is_contiguous()
    verts, cam_t, focal = _rows(dev, [[-0.15, 0.0, 3.0], [0.2, 0.05, 3.15], [1.0, 0.0, 2.5], [0.02, 0.0, 0.15]], [sizes[i] for i in index])
    r = MeshRenderer(FACES)
    want = {}
    for i in (0, 2):
        rows = [p for p, f in enumerate(index) if f == i]
        want[i] = {pp: r.render(frames[i], verts[rows], cam_t[rows], focal[rows], per_person=pp, want=('face', 'depth', 'color')) for pp in (False, True)}
    return dict(r=r, sizes=sizes, index=index, frames=frames, verts=verts, cam_t=cam_t, focal=focal, want=want)


def test_clip_overlay_equals_the_per_frame_renderer(dev, scene):
    s = scene
    out = s['r'].render_clip(s['frames'], s['verts'], s['cam_t'], s['focal'], s['index'], want=('face', 'depth', 'color'))
    assert len(out['image']) == 3 and [tuple(i.shape) for i in out['image']] == [hw + (3,) for hw in s['sizes']]
    assert torch.equal(out['image'][1], s['frames'][1]) and (out['face'][1] == -1).all() and not out['depth'][1].any()      # the empty frame: its own bytes
    for i, first_row in ((0, 0), (2, 2)):
        ref = s['want'][i][False]
        assert torch.equal(out['image'][i], ref['image']), i
        assert torch.equal(out['depth'][i], ref['depth']) and torch.equal(out['color'][i], ref['color']), i
        face = torch.where(out['face'][i] >= 0, out['face'][i] - first_row * NF, out['face'][i])
        assert torch.equal(face, ref['face']), i
    # the scene shows what it is meant to: both persons of frame 0 visible, frame 2 drawn up to its right border, faces dropped at znear
    f0, f2 = s['want'][0][False]['face'], s['want'][2][False]['face']
    assert ((f0 >= 0) & (f0 < NF)).sum() > 50 and (f0 >= NF).sum() > 50 and (f2[:, -1] >= 0).any()
    near = s['r'].render(s['frames'][2], s['verts'][3:4], s['cam_t'][3:4], s['focal'][3:4], want=('screen', 'face'))
    assert (near['screen'][..., 2] <= 0.05).any() and (near['screen'][..., 2] > 0.05).any()
    # plain call: the images alone; a CPU tensor and a numpy array as frame_index
    plain = s['r'].render_clip(s['frames'], s['verts'], s['cam_t'], s['focal'], torch.tensor(s['index']))
    again = s['r'].render_clip(s['frames'], s['verts'], s['cam_t'], s['focal'], np.asarray(s['index']))
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(plain, out['image'], again))
    with pytest.raises(RuntimeError, match='frame_index'):
        s['r'].render_clip(s['frames'], s['verts'], s['cam_t'], s['focal'], torch.tensor(s['index'], device=dev))


def test_one_tensor_of_frames_gives_views_of_one_tensor(dev, scene):
    s = scene
    frames = torch.stack(_frames(dev, [(48, 64)] * 3, 12))
    rows = [0, 1]
    imgs = s['r'].render_clip(frames, s['verts'][rows], s['cam_t'][rows], s['focal'][rows], [2, 2], centers=[(32, 24), (30, 20), (33.5, 25.25)])
    assert len(imgs) == 3 and imgs[1].data_ptr() - imgs[0].data_ptr() == 48 * 64 * 3
    assert torch.equal(imgs[0], frames[0]) and torch.equal(imgs[1], frames[1])
    assert torch.equal(imgs[2], s['r'].render(frames[2], s['verts'][rows], s['cam_t'][rows], s['focal'][rows], center=(33.5, 25.25)))


def test_wave_path_and_lane_path_in_one_call(dev, scene):
    """a close person (faces of hundreds of pixels: the whole-wave walk) and, in a frame of another size, a distant one (faces of one or two pixels:
    the lane walk); the 84 faces per draw put both kinds into one wave"""
    r = scene['r']
    sizes = [(96, 128), (50, 70)]
    frames = _frames(dev, sizes, 13)
    verts, cam_t, focal = _rows(dev, [[0.05, 0.0, 1.5], [0.3, -0.2, 12.0]], sizes)
    out = r.render_clip(frames, verts, cam_t, focal, [0, 1], want=('face',))
    for i in (0, 1):
        ref = r.render(frames[i], verts[i:i + 1], cam_t[i:i + 1], focal[i:i + 1], want=('face',))
        assert torch.equal(out['image'][i], ref['image']), i
        assert torch.equal(torch.where(out['face'][i] >= 0, out['face'][i] - i * NF, out['face'][i]), ref['face']), i
    per_face = [torch.bincount(out['face'][i][out['face'][i] >= 0] - i * NF, minlength=NF) for i in (0, 1)]
    assert (per_face[0] > 16).sum() > 10                       # more than MESH_SMALL pixels already visible, so the boxes are larger still
    assert 0 < per_face[1].max() <= 8 and per_face[1].sum() > 5       # an ellipse of 1.8 x 5 pixels half axes: a face box stays far below MESH_SMALL


def test_depth_ties_go_to_the_earlier_draw(dev, scene):
    r = scene['r']
    sizes = [(48, 64), (40, 56)]
    frames = _frames(dev, sizes, 14)
    verts, cam_t, focal = _rows(dev, [[0.1, 0.0, 3.0], [0.1, 0.0, 3.0], [0.0, 0.1, 2.8]], [sizes[0], sizes[0], sizes[1]])
    verts[1] = verts[0]                                        # rows 0 and 1: the same person twice, every pixel a tie
    a = r.render_clip(frames, verts, cam_t, focal, [0, 0, 1], want=('face',))
    fa = a['face'][0]
    assert (fa >= 0).sum() > 100 and (fa[fa >= 0] < NF).all()
    assert torch.equal(a['image'][0], r.render(frames[0], verts[:1], cam_t[:1], focal[:1]))
    order = [2, 0, 1]                                          # the same rows in another order: frame 0 is now drawn by rows 1 and 2
    b = r.render_clip(frames, verts[order], cam_t[order], focal[order], [1, 0, 0], want=('face',))
    fb = b['face'][0]
    assert torch.equal(b['image'][0], a['image'][0]) and torch.equal(b['image'][1], a['image'][1])
    assert torch.equal(fb >= 0, fa >= 0) and ((fb[fb >= 0] >= NF) & (fb[fb >= 0] < 2 * NF)).all()
    assert torch.equal(fb[fb >= 0] - NF, fa[fa >= 0])


def test_per_person_images(dev, scene):
    s = scene
    out = s['r'].render_clip(s['frames'], s['verts'], s['cam_t'], s['focal'], s['index'], per_person=True, want=('face', 'depth'))
    assert len(out['image']) == 4
    ref_img = [im for i in (0, 2) for im in s['want'][i][True]['image']]
    ref_depth = [d for i in (0, 2) for d in s['want'][i][True]['depth']]
    ref_face = [f for i in (0, 2) for f in s['want'][i][True]['face']]
    for p in range(4):
        assert torch.equal(out['image'][p], ref_img[p]) and torch.equal(out['depth'][p], ref_depth[p]), p
        first_row = 0 if p < 2 else 2
        assert torch.equal(torch.where(out['face'][p] >= 0, out['face'][p] - first_row * NF, out['face'][p]), ref_face[p]), p
    plain = s['r'].render_clip(s['frames'], s['verts'], s['cam_t'], s['focal'], s['index'], per_person=True)
    assert all(torch.equal(a, b) for a, b in zip(plain, ref_img))


def test_strips_equal_render_image_group(dev, scene):
    from whmr_amd.utils.renderer_cam import render_clip_groups, render_image_group
    r = scene['r']
    H, W = 48, 64
    frames = torch.stack(_frames(dev, [(H, W)] * 2, 15))
    index = [0, 1, 1]
    local, cam_t, focal = _rows(dev, [[-0.1, 0.0, 3.0], [0.3, 0.1, 2.6], [-0.4, 0.0, 3.4]], [(H, W)] * 3)
    world = (local @ torch.from_numpy(MR.rotation((0.0, 1.0, 0.2), 25.0).astype(np.float32)).to(dev).T).contiguous()     # smpl_vertices: another orientation
    strips = render_clip_groups(frames, cam_t, world, local, np.eye(3), focal, index, r)
    assert len(strips) == 3 and strips[1].data_ptr() - strips[0].data_ptr() == H * 4 * W * 3
    for p, i in enumerate(index):
        fl = (float(focal[p]), float(focal[p]))
        ref = render_image_group(frames[i], cam_t[p], world[p], local[p], np.eye(3), fl, (W // 2, H // 2), r)
        assert strips[p].shape == (H, 4 * W, 3) and torch.equal(strips[p], ref), p
        assert torch.equal(strips[p][:, :W], frames[i]) and (strips[p][:, W:2 * W] != frames[i]).any()
        assert strips[p][:, 2 * W:3 * W].any() and not torch.equal(strips[p][:, 2 * W:3 * W], strips[p][:, 3 * W:])


def test_capture_in_a_hip_graph_replays_the_eager_bits(dev, scene):
    """fixed tables, one stream: the launch group allocates nothing outside torch's (capturable) allocator and never synchronises; new vertices in the
    captured buffers give the eager picture of the new vertices"""
    s, r = scene, scene['r']
    verts, cam_t = s['verts'].contiguous(), s['cam_t'].contiguous()
    focal = s['focal'].reshape(-1, 1).expand(-1, 2).contiguous()
    moved_verts = verts + torch.tensor([0.05, -0.03, 0.1], device=dev)
    eager = r.render_clip(s['frames'], verts, cam_t, focal, s['index'], want=('face',))
    moved = r.render_clip(s['frames'], moved_verts, cam_t, focal, s['index'], want=('face',))
    assert not torch.equal(moved['image'][0], eager['image'][0])
    backgrounds = s['frames']
    outputs = [torch.zeros(hw + (3,), dtype=torch.uint8, device=dev) for hw in s['sizes']]
    images, table, total = r.plan_draws(s['sizes'], [(row, 0, i, 0.0) for row, i in enumerate(s['index'])], frame_strides=[b.stride(0) for b in backgrounds],
                                        n_rows=4)
    tables = r.upload_draws(images, table, backgrounds, outputs, dev)
    sv = verts.clone()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):
        r.run_draws(tables, 3, 4, total, sv, None, cam_t, focal, want=('face',))          # warm-up on the capture stream: tables and workspace exist
    torch.cuda.current_stream().wait_stream(cs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        cap = r.run_draws(tables, 3, 4, total, sv, None, cam_t, focal, want=('face',))
    offs = images['pix_off'].tolist()
    for want in (eager, moved):
        for o in outputs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for i, (h, w) in enumerate(s['sizes']):
            assert torch.equal(outputs[i], want['image'][i]), i
            assert torch.equal(cap['face'][offs[i]:offs[i] + h * w].view(h, w), want['face'][i]), i
        r.render_clip([torch.zeros(200, 300, 3, dtype=torch.uint8, device=dev)], verts[:1], cam_t[:1], focal[:1], [0])     # a larger eager call beside it
        sv.copy_(moved_verts)


@pytest.fixture(scope='module')
def model(dev, assets, state_dict):
    from whmr_amd.models import whmr_net
    m = whmr_net(None, assets=assets, numerics='bf16')
    m.load_state_dict(state_dict, strict=False)
    return m.to(dev).eval()


def test_clip_pipeline_draws_the_clip_in_one_call(dev, model):
    from whmr_amd.demo import ClipPipeline, render_frame
    from whmr_amd.utils.renderer_cam import MeshRenderer
    r = MeshRenderer(MR.uv_sphere()[1])
    frames = torch.from_numpy(np.random.default_rng(16).integers(0, 256, size=(3, 90, 120, 3), dtype=np.uint8)).to(dev)
    dets = [[(50.0, 40.0, 60.0, 60.0)], [], [(90.5, 30.0, 44.0, 44.0), (60.0, 50.0, 70.0, 70.0)]]
    pipe = ClipPipeline(model, renderer=r)
    out, images = pipe(frames, dets)
    assert len(images) == 3 and out['frame_index'].tolist() == [0, 2, 2]
    keys = ('local_smpl_vertices', 'pred_cam_t', 'focal_length')
    for i, rows in ((0, slice(0, 1)), (2, slice(1, 3))):
        assert torch.equal(images[i], render_frame({k: out[k][rows] for k in keys}, frames[i], r)), i
    assert torch.equal(images[1], frames[1])
    assert ClipPipeline(model, renderer=r, per_person=True).per_person and not pipe.per_person
    pipe.per_person = True                                     # the same pipeline and graph, one image per person
    out2, per = pipe(frames, dets)
    assert len(per) == 3 and len(pipe._graphs) == 1 and all(torch.equal(out2[k], out[k]) for k in keys)
    ref = [render_frame({k: out[k][0:1] for k in keys}, frames[0], r, per_person=True), render_frame({k: out[k][1:3] for k in keys}, frames[2], r, per_person=True)]
    assert all(torch.equal(a, b) for a, b in zip(per, torch.cat(ref)))
