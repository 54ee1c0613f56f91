"""Mesh overlay renderer on the device (csrc/mesh_render.hip, whmr_amd.utils.renderer_cam) against its float64 restatement
(tests/mesh_render_reference.py) and the analytic known answers."""
import numpy as np
import pytest
import torch

import mesh_render_reference as MR
from conftest import ew_err

pytestmark = pytest.mark.gpu

# camera of the single-triangle cases: f = 128 at depth 2 around centre (24, 24) puts x = (u - 24) / 64 on pixel coordinate u exactly, in fp32 too
F0, D0, C0, S0 = 128.0, 2.0, 24.0, 48


def _pt(u, v, z=D0):
    return [(u - C0) * z / F0, (v - C0) * z / F0, z]


def _render(dev, renderer, verts, cam_t=None, per_person=False, want=('face', 'color', 'depth'), frame=None):
    verts = torch.tensor(verts, dtype=torch.float32)
    P = verts.shape[0]
    cam_t = torch.zeros(P, 3) if cam_t is None else torch.tensor(cam_t, dtype=torch.float32)
    frame = torch.full((S0, S0, 3), 77, dtype=torch.uint8) if frame is None else frame
    return renderer.render(frame.to(dev), verts.to(dev), cam_t.to(dev), torch.full((P,), F0).to(dev), center=(C0, C0), per_person=per_person, want=want)


def test_single_triangles(dev):
    from whmr_amd.utils.renderer_cam import MeshRenderer
    yy, xx = np.mgrid[0:S0, 0:S0] + 0.5
    tri = lambda z: [_pt(10.5, 10.5, z), _pt(30.5, 10.5, z), _pt(10.5, 30.5, z)]
    # top-left rule on the triangle with corners on pixel centres: left and top edge owned, the hypotenuse (a right / bottom edge) not
    expect = (xx >= 10.5) & (yy >= 10.5) & ((xx - 10.5) + (yy - 10.5) < 20)
    # the nearer one wins in either face order
    for faces in ([[0, 1, 2], [3, 4, 5]], [[3, 4, 5], [0, 1, 2]]):
        out = _render(dev, MeshRenderer(faces), [tri(3.0) + tri(2.5)])
        fid = out['face'].cpu().numpy()
        assert np.array_equal(fid >= 0, expect) and (fid[expect] == faces.index([3, 4, 5])).all()
        assert np.allclose(out['depth'].cpu().numpy()[expect], 2.5, rtol=1e-5) and not out['depth'].cpu().numpy()[~expect].any()
        ref, rdepth, _ = MR.rasterize(MR.project(np.array([tri(3.0) + tri(2.5)]), np.zeros((1, 3)), [[F0, F0]], (C0, C0)), np.asarray(faces), S0, S0)
        assert np.array_equal(fid, ref[0])
    # equal depth: the smaller global face id, within a person and across persons
    r2 = MeshRenderer([[3, 4, 5], [0, 1, 2]])
    assert (_render(dev, r2, [tri(2.5) + tri(2.5)])['face'].cpu().numpy()[expect] == 0).all()
    two = [tri(2.5) + tri(9.0), tri(7.0) + tri(2.5)]                     # person 0's face 1 (id 1) ties with person 1's face 0 (id 2)
    fid = _render(dev, r2, two)['face'].cpu().numpy()
    assert np.array_equal(fid >= 0, expect) and (fid[expect] == 1).all()
    fid = _render(dev, r2, two, per_person=True)['face'].cpu().numpy()
    assert fid.shape == (2, S0, S0) and (fid[0][expect] == 1).all() and (fid[1][expect] == 2).all() and (fid[:, ~expect] == -1).all()
    # the same through the per-person translation instead of the vertices
    back = [[x, y, 1.0] for x, y, _ in tri(2.5)]                         # x, y of depth 2.5, 1.5 of it supplied by cam_t
    fid = _render(dev, r2, [back + back] * 2, cam_t=[[0, 0, 1.5], [0, 0, 1.5]])['face'].cpu().numpy()
    assert np.array_equal(fid >= 0, expect) and (fid[expect] == 0).all()
    # shared edge: a square split along either diagonal, either winding, covers every centre once (left / top border in, right / bottom out)
    sq = [[_pt(10.5, 10.5), _pt(30.5, 10.5), _pt(30.5, 30.5), _pt(10.5, 30.5)]]
    inside = (xx >= 10.5) & (xx < 30.5) & (yy >= 10.5) & (yy < 30.5)
    for faces in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 3, 2]], [[0, 1, 3], [1, 2, 3]], [[2, 1, 0], [0, 2, 3]]):
        both = _render(dev, MeshRenderer(faces), sq)['face'].cpu().numpy()
        one = [_render(dev, MeshRenderer([f]), sq)['face'].cpu().numpy() >= 0 for f in faces]
        assert np.array_equal(one[0].astype(int) + one[1].astype(int), inside.astype(int)), faces
        assert np.array_equal(both >= 0, inside) and np.array_equal(both == 0, one[0])
        ref, _, _ = MR.rasterize(MR.project(np.array(sq), np.zeros((1, 3)), [[F0, F0]], (C0, C0)), np.asarray(faces), S0, S0)
        assert np.array_equal(both, ref[0])
    # a face behind znear is dropped whole (one vertex is enough)
    near = [_pt(10.5, 10.5, 0.04), _pt(30.5, 10.5, 2.5), _pt(10.5, 30.5, 2.5)]
    fid = _render(dev, MeshRenderer([[0, 1, 2], [3, 4, 5]]), [near + tri(3.0)])['face'].cpu().numpy()
    assert np.array_equal(fid >= 0, expect) and (fid[expect] == 1).all()
    # NaN and far off-screen vertices change nothing (and fault nothing); the frame shows through bit for bit
    base = _render(dev, MeshRenderer([[0, 1, 2]]), [tri(2.5)], want=('face', 'color'))
    nan, far, inf = float('nan'), 1e30, float('inf')
    junk = tri(2.5) + [[nan, 0, 2], [0, 0, 2], [1, 0, 2]] + [[far, far, 2], [far, -far, 2], [-far, 0, 2]] + [[0, 0, nan], [1, 0, 2], [0, 1, 2]] \
        + [[inf, 0, 2], [0, -inf, 2], [0, 0, 2]] + [[5, 5, 2], [6, 5, 2], [5, 6, 2]] + [[0, 0, -3], [1, 0, -3], [0, 1, -3]]
    out = _render(dev, MeshRenderer([[3, 4, 5], [6, 7, 8], [0, 1, 2], [9, 10, 11], [12, 13, 14], [15, 16, 17], [18, 19, 20]]), [junk], want=('face', 'color'))
    fid = out['face'].cpu().numpy()
    assert np.array_equal(fid >= 0, expect) and (fid[expect] == 2).all()
    assert torch.equal(out['color'], base['color']) and torch.equal(out['image'], base['image'])
    assert (out['image'].cpu().numpy()[~expect] == 77).all()
    torch.cuda.synchronize()


@pytest.mark.parametrize('size', [(720, 1280), (487, 653)])
def test_three_persons_against_the_float64_reference(dev, size):
    """Three ellipsoid persons of SMPL's vertex / face counts (two interpenetrating, one cut by the border), both per_person modes.
    Bounds: face id differs on < 2e-3 of the pixels (the cap tests/test_raster_gpu.py gives fp32-vs-float64 edge decisions; the reference in float32
    against itself in float64 differs on 5.4e-6 / 0 of the pixels of the two scenes, tests/test_mesh_render_cpu.py); fp32 colour on agreeing pixels:
    max < 1e-3, median < 1e-6 (test_raster_gpu.py's bounds for barycentric-interpolated values; the reference's own float32-vs-float64 colour error
    on these scenes is max 6.2e-5, median 4.7e-8, so the median bound is reachable with the renormalised normal and is kept as it stands).
    Measured on the device: face id differs on 5.4e-6 / 1.8e-6 (720 x 1280, shared / per person) and 0 (487 x 653) of the pixels, colour max 7.0e-5,
    median 4.7e-8."""
    from whmr_amd.utils.renderer_cam import MeshRenderer, DEFAULT_COLOR
    H, W = size
    verts, faces, cam_t, focal = MR.three_person_scene(H, W)
    frame = np.random.default_rng(1).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    r = MeshRenderer(faces)
    dv, dt, df, dfr = torch.from_numpy(verts).to(dev), torch.from_numpy(cam_t).to(dev), torch.from_numpy(focal).to(dev), torch.from_numpy(frame).to(dev)
    for per_person in (False, True):
        out = r.render(dfr, dv, dt, df, per_person=per_person, want=('face', 'color', 'depth', 'screen'))
        ref = MR.render(frame, verts, faces, cam_t, focal, per_person=per_person, base=DEFAULT_COLOR)
        fid, col, img = out['face'].cpu().numpy(), out['color'].cpu().numpy(), out['image'].cpu().numpy()
        assert img.shape == ((3, H, W, 3) if per_person else (H, W, 3)) and img.dtype == np.uint8
        covered = (ref['face'] >= 0).mean()
        differ = (fid != ref['face']).mean()
        agree = (fid == ref['face']) & (fid >= 0)
        err = np.abs(col.astype(np.float64) - ref['color'])[agree]
        print('%dx%d per_person=%s: covered %.3f; face id differs on %.2e of the pixels; colour error on agreeing pixels max %.2e median %.2e'
              % (H, W, per_person, covered, differ, err.max(), np.median(err)))
        assert covered > 0.02
        assert differ < 2e-3
        assert err.max() < 1e-3 and np.median(err) < 1e-6
        derr = np.abs(out['depth'].cpu().numpy() - ref['depth'])[agree]
        assert derr.max() < 1e-4
        # uint8: round(255 colour) of the device's own fp32 colour exactly; within one level of the reference where the face agrees
        mine = torch.round(255 * out['color']).to(torch.uint8)
        cov = (out['face'] >= 0).unsqueeze(-1)
        assert torch.equal(torch.where(cov, out['image'], torch.zeros_like(out['image'])), torch.where(cov, mine, torch.zeros_like(mine)))
        assert np.abs(img.astype(int) - ref['image'].astype(int))[agree].max() <= 1
        # background: the frame's bytes
        bg = fid < 0
        assert np.array_equal(img[bg], np.broadcast_to(frame, img.shape)[bg]) and not col[bg].any()
        # screen-space vertices: the package's perspective projection
        from whmr_amd.utils.geometry import perspective_projection
        pp = perspective_projection(dv, torch.eye(3, device=dev)[None], dt, df, torch.tensor([[W // 2, H // 2]], dtype=torch.float32, device=dev).expand(3, 2).contiguous())
        assert ew_err(out['screen'][..., :2], pp) < 1e-4
        assert ew_err(out['screen'], ref['screen']) < 1e-4
        # two runs give identical bits (overlapping persons included)
        again = r.render(dfr, dv, dt, df, per_person=per_person, want=('face', 'color', 'depth'))
        assert all(torch.equal(out[k], again[k]) for k in ('image', 'face', 'color', 'depth'))
    # shared depth buffer vs one person per image: person 1 loses pixels to person 0 only where they overlap
    Fn = faces.shape[0]
    shared = r.render(dfr, dv, dt, df, want=('face',))['face']
    each = r.render(dfr, dv, dt, df, per_person=True, want=('face',))['face']
    assert ((shared // Fn == 1) & (shared >= 0)).sum() < (each[1] >= 0).sum() and ((shared >= 0) == (each >= 0).any(0)).all()


def test_side_view_and_camera_rotation_against_the_reference(dev):
    from whmr_amd.utils.renderer_cam import MeshRenderer, DEFAULT_COLOR
    H, W = 240, 320
    verts, faces, cam_t, focal = MR.three_person_scene(H, W)
    frame = np.zeros((H, W, 3), np.uint8)
    rot = MR.rotation((0.2, 1.0, 0.1), 9.0)
    r = MeshRenderer(faces)
    dv, dt, df = torch.from_numpy(verts[:2]).to(dev), torch.from_numpy(cam_t[:2]).to(dev), torch.from_numpy(focal[:2]).to(dev)
    for kw in (dict(sideview_angle=270), dict(rot=rot), dict(rot=rot, sideview_angle=90)):
        out = r.render(None, dv, dt, df, size=(H, W), want=('face', 'color'), **{k: (torch.from_numpy(v) if k == 'rot' else v) for k, v in kw.items()})
        ref = MR.render(frame, verts[:2], faces, cam_t[:2], focal[:2], base=DEFAULT_COLOR, **kw)
        fid = out['face'].cpu().numpy()
        agree = (fid == ref['face']) & (fid >= 0)
        err = np.abs(out['color'].cpu().numpy() - ref['color'])[agree]
        print(kw.keys(), 'covered %.3f differ %.2e colour max %.2e median %.2e' % ((fid >= 0).mean(), (fid != ref['face']).mean(), err.max(), np.median(err)))
        assert (ref['face'] >= 0).mean() > 0.02 and (fid != ref['face']).mean() < 2e-3 and err.max() < 1e-3 and np.median(err) < 1e-6
        assert not out['image'].cpu().numpy()[fid < 0].any()


def test_render_image_group(dev):
    from whmr_amd.utils.renderer_cam import MeshRenderer, render_image_group, render_overlay_image
    H, W = 180, 240
    verts, faces, cam_t, focal = MR.three_person_scene(H, W)
    frame = torch.from_numpy(np.random.default_rng(2).integers(1, 256, size=(H, W, 3), dtype=np.uint8)).to(dev)
    r = MeshRenderer(faces, color=(0.9, 0.5, 0.4))
    local, world = torch.from_numpy(verts[0]).to(dev), torch.from_numpy(verts[1]).to(dev)
    t = torch.from_numpy(cam_t[0]).to(dev)
    t0 = t.clone()
    fl = (float(focal[0]), float(focal[0]))
    strip = render_image_group(frame, t, world, local, np.eye(3), fl, (W // 2, H // 2), r)
    assert strip.shape == (H, 4 * W, 3) and strip.dtype == torch.uint8 and torch.equal(t, t0)
    assert torch.equal(strip[:, :W], frame)
    over = render_overlay_image(frame, t, local, np.eye(3), fl, (W // 2, H // 2), r)
    assert torch.equal(strip[:, W:2 * W], over) and (over != frame).any(-1).float().mean() > 0.02
    for k, v in ((2, local), (3, world)):
        side = r.render(None, v[None], t[None], torch.tensor([fl], device=dev), size=(H, W), sideview_angle=270, want=('face',))
        panel = strip[:, k * W:(k + 1) * W]
        assert torch.equal(panel, side['image']) and (side['face'] >= 0).float().mean() > 0.01
        assert not panel[side['face'] < 0].any()                                      # black outside the mesh
        assert (panel[side['face'] >= 0].float().sum(-1) > 0).all()


def test_capture_in_a_hip_graph_replays_the_eager_bits(dev):
    """one stream, no parallel branches: the call allocates nothing outside torch's (capturable) allocator and never synchronises"""
    from whmr_amd.utils.renderer_cam import MeshRenderer
    H, W = 360, 640
    verts, faces, cam_t, focal = MR.three_person_scene(H, W)
    r = MeshRenderer(faces)
    frame = torch.from_numpy(np.random.default_rng(4).integers(0, 256, size=(H, W, 3), dtype=np.uint8)).to(dev)
    dv, dt, df = torch.from_numpy(verts).to(dev), torch.from_numpy(cam_t).to(dev), torch.from_numpy(focal).to(dev)
    eager = r.render(frame, dv, dt, df, want=('face', 'color'))
    moved = r.render(frame, dv, dt + torch.tensor([0.2, 0.0, 0.3], device=dev), df, want=('face',))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r.render(frame, dv, dt, df, want=('face', 'color'))                              # warm-up on the capture stream: tables and workspace exist
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    sv, st = dv.clone(), dt.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap = r.render(frame, sv, st, df, want=('face', 'color'))
    for _ in range(2):
        cap['image'].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(cap[k], eager[k]) for k in ('image', 'face', 'color'))
    st.copy_(dt + torch.tensor([0.2, 0.0, 0.3], device=dev))                             # new inputs in the captured buffers: a new picture
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap['face'], moved['face']) and not torch.equal(cap['face'], eager['face'])


def test_frame_pipeline_returns_the_picture(dev, assets, state_dict):
    from whmr_amd.demo import FramePipeline, render_frame
    from whmr_amd.models import whmr_net
    from whmr_amd.utils.renderer_cam import MeshRenderer
    _, faces = MR.uv_sphere()
    rng = np.random.default_rng(3)
    frame = torch.from_numpy(rng.integers(0, 256, size=(360, 640, 3), dtype=np.uint8)).to(dev)
    frame2 = torch.from_numpy(rng.integers(0, 256, size=(360, 640, 3), dtype=np.uint8)).to(dev)
    dets = [(320.0, 180.0, 220.0, 220.0), (100.5, 90.0, 150.0, 150.0)]
    m = whmr_net(None, assets=assets, numerics='bf16')
    m.load_state_dict(state_dict, strict=False)
    m = m.to(dev).eval()
    plain = FramePipeline(m)
    want = {k: v.clone() for k, v in plain(frame, dets).items()}
    r = MeshRenderer(faces)
    pipe = FramePipeline(m, renderer=r)
    out, img = pipe(frame, dets)
    assert set(out) == set(want) and all(torch.equal(out[k], want[k]) for k in want)
    assert img.shape == (360, 640, 3) and img.dtype == torch.uint8
    covered = (img != frame).any(-1).float().mean().item()
    print('pipeline picture: %.3f of the pixels drawn; pred_cam_t' % covered, out['pred_cam_t'].cpu().tolist())
    assert covered > 0
    assert torch.equal(img, render_frame(out, frame, r))
    out2, img2 = pipe(frame2, [(300.0, 200.0, 200.0, 200.0), (500.0, 120.0, 160.0, 160.0)])
    assert len(pipe._graphs) == 1 and img2.shape == img.shape and all(torch.isfinite(v).all() for v in out2.values())
    assert torch.equal(img2, render_frame(out2, frame2, r))
    per = FramePipeline(m, renderer=r, per_person=True)
    assert per(frame, dets)[1].shape == (2, 360, 640, 3)
