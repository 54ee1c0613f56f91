"""The float64 restatement of the mesh overlay renderer (tests/mesh_render_reference.py) pinned on known answers, the rounding condition of the device
test's face-id cap, and the loud failure of MeshRenderer.render without a HIP device."""
import math

import numpy as np
import pytest
import torch

import mesh_render_reference as MR


def test_test_mesh_has_smpl_counts_and_is_closed_and_wound_outwards():
    v, f = MR.uv_sphere()
    assert v.shape == (6890, 3) and f.shape == (13776, 3) and f.min() == 0 and f.max() == 6889
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fwd = {(a, b) for a, b in e.tolist()}
    assert len(fwd) == len(e) and all((b, a) in fwd for a, b in fwd)              # every directed edge once, its opposite present: closed, consistent
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.einsum('ij,ij->i', n, v[f].mean(1)) > 0).all()                      # every face normal points away from the centre


def test_sphere_covers_the_disc_of_its_tangent_cone():
    """a centred sphere of radius r at depth d covers the disc of radius f r / sqrt(d^2 - r^2); the inscribed polyhedron covers at least the disc of
    its own inscribed sphere (radius rho r, rho from the mesh's face planes); a pixel square reaches sqrt(2) / 2 from its centre"""
    v, f = MR.uv_sphere()
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    rho = (np.einsum('ij,ij->i', n, v[f[:, 0]]) / np.linalg.norm(n, axis=1)).min()
    assert 0.99 < rho < 1
    r, d, foc, H, W = 0.5, 3.0, 400.0, 201, 241
    frame = np.zeros((H, W, 3), np.uint8)
    out = MR.render(frame, (v * r)[None], f, [[0.0, 0.0, d]], [foc], center=(W / 2, H / 2))
    count = int((out['face'] >= 0).sum())
    R_out, R_in = foc * r / math.sqrt(d * d - r * r), foc * rho * r / math.sqrt(d * d - (rho * r) ** 2)
    lo, hi = math.pi * (R_in - math.sqrt(0.5)) ** 2, math.pi * (R_out + math.sqrt(0.5)) ** 2
    print('sphere: %d pixels, disc %.1f (bounds %.1f .. %.1f)' % (count, math.pi * R_out ** 2, lo, hi))
    assert lo <= count <= hi
    yy, xx = np.mgrid[0:H, 0:W] + 0.5
    rr = np.hypot(xx - W / 2, yy - H / 2)
    assert (out['face'] >= 0)[rr < R_in - 1e-9].all() and not (out['face'] >= 0)[rr > R_out + 1e-9].any()
    assert np.allclose(out['depth'][H // 2, W // 2], d - r, atol=2e-3 * r)       # the nearest point, up to the tessellation


def test_projection_is_the_packages_perspective_projection():
    from oracle import geometry as OG
    g = np.random.default_rng(0)
    pts = g.normal(size=(3, 50, 3)) * 0.4
    t = np.array([[0.1, -0.2, 3.0], [-0.4, 0.3, 5.5], [0.0, 0.0, 2.2]])
    foc = np.array([1000.0, 1468.6, 700.0])
    scr = MR.project(pts, t, np.stack([foc, foc], 1), (320.0, 180.0))
    ref = OG.perspective_projection(torch.from_numpy(pts), torch.eye(3, dtype=torch.float64)[None], torch.from_numpy(t), torch.from_numpy(foc),
                                    torch.tensor([[320.0, 180.0]], dtype=torch.float64).expand(3, 2))
    assert np.abs(scr[..., :2] - ref.numpy()).max() < 1e-9
    assert np.allclose(scr[..., 2], pts[..., 2] + t[:, None, 2], atol=1e-12)


def test_shared_diagonal_is_covered_exactly_once():
    """a square with corners on pixel centres, split along its diagonal: the diagonal's centres belong to exactly one triangle, the left and top
    border to the square, the right and bottom border not (top-left rule) -- for both windings and both diagonals"""
    yy, xx = np.mgrid[0:48, 0:48] + 0.5
    expect = (xx >= 10.5) & (xx < 30.5) & (yy >= 10.5) & (yy < 30.5)
    sq = np.array([[[10.5, 10.5, 2.0], [30.5, 10.5, 2.0], [30.5, 30.5, 2.0], [10.5, 30.5, 2.0]]])
    for faces in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 3, 2]], [[0, 1, 3], [1, 2, 3]], [[2, 1, 0], [0, 2, 3]]):
        faces = np.asarray(faces, np.int32)
        both, _, _ = MR.rasterize(sq, faces, 48, 48)
        one = [MR.rasterize(sq, faces[k:k + 1], 48, 48)[0][0] >= 0 for k in range(2)]
        assert np.array_equal(one[0].astype(int) + one[1].astype(int), expect.astype(int)), faces.tolist()
        assert np.array_equal(both[0] >= 0, expect)
        assert one[0].sum() > 150 and one[1].sum() > 150


def test_nearest_face_wins_and_ties_go_to_the_smaller_global_id():
    tri = lambda z: [[10.5, 10.5, z], [30.5, 10.5, z], [10.5, 30.5, z]]
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    fid, depth, _ = MR.rasterize(np.array([tri(3.0) + tri(2.5)]), faces, 40, 40)
    assert set(np.unique(fid)) == {-1, 1} and np.allclose(depth[fid == 1], 2.5)
    fid, _, _ = MR.rasterize(np.array([tri(2.5) + tri(2.5)]), faces, 40, 40)
    assert set(np.unique(fid)) == {-1, 0}
    two = np.array([tri(2.5) + tri(9.0), tri(7.0) + tri(2.5)])                     # person 1's second face ties with person 0's first
    fid, _, _ = MR.rasterize(two, faces, 40, 40)
    assert set(np.unique(fid)) == {-1, 0}
    fid, _, _ = MR.rasterize(two, faces, 40, 40, per_person=True)
    assert set(np.unique(fid[0])) == {-1, 0} and set(np.unique(fid[1])) == {-1, 3}
    fid, _, _ = MR.rasterize(np.array([tri(0.04) + tri(2.5)]), faces, 40, 40)      # behind znear: dropped whole
    assert set(np.unique(fid)) == {-1, 1}


def test_pole_on_shade():
    """the sphere point nearest to the camera has its normal along the light: colour = base (ambient + k_d)"""
    v, f = MR.uv_sphere()
    v = v @ MR.rotation((1.0, 0.0, 0.0), -90.0).T                                  # pole (0, 1, 0) -> (0, 0, -1): towards the camera
    assert np.allclose(v[0], [0, 0, -1])
    base = (0.5, 0.6, 0.7)
    out = MR.render(np.zeros((65, 65, 3), np.uint8), (v * 0.4)[None], f, [[0.0, 0.0, 2.0]], [300.0], center=(32.5, 32.5), base=base)
    want = np.asarray(base) * (MR.AMBIENT + MR.K_D)
    assert want.max() < 1 and abs(MR.K_D - 0.97785) < 1e-5
    assert np.abs(out['color'][32, 32] - want).max() < 1e-9
    assert np.array_equal(out['image'][32, 32], np.round(255 * want).astype(np.uint8))
    assert (out['color'][out['face'] >= 0] >= np.asarray(base) * MR.AMBIENT - 1e-12).all()        # never darker than the ambient term


def test_side_view_is_a_rotation_of_the_mesh():
    verts, f, cam_t, focal = MR.three_person_scene(90, 120)
    verts, cam_t, focal = verts[2:].astype(np.float64), np.array([[0.1, 0.0, 3.0]]), focal[:1]
    frame = np.zeros((90, 120, 3), np.uint8)
    a = MR.render(frame, verts, f, cam_t, focal, sideview_angle=270)
    D = np.diag([1.0, -1.0, -1.0])
    byhand = verts @ (D @ MR.rot_y(270) @ D).T
    b = MR.render(frame, byhand, f, cam_t, focal)
    assert (a['face'] >= 0).mean() > 0.02
    assert (a['face'] != b['face']).mean() < 1e-3 and np.abs(a['color'] - b['color'])[a['face'] == b['face']].max() < 1e-9
    c = MR.render(frame, verts, f, cam_t, focal)
    assert (a['face'] != c['face']).mean() > 0.01                                   # and it is not the front view


@pytest.mark.parametrize('size', [(720, 1280), (487, 653)])
def test_rounding_alone_stays_below_half_the_face_id_cap(size):
    """condition of the device test's 2e-3 cap on differing face ids: the same arithmetic in float32 against float64 on the chosen scene differs on
    less than half of it (otherwise the scene moves, not the cap).  Also prints the float32-vs-float64 colour error on agreeing pixels."""
    H, W = size
    verts, f, cam_t, focal = MR.three_person_scene(H, W)
    frame = np.zeros((H, W, 3), np.uint8)
    a = MR.render(frame, verts, f, cam_t, focal)
    b = MR.render(frame, verts, f, cam_t, focal, dtype=np.float32)
    differ = (a['face'] != b['face']).mean()
    agree = (a['face'] == b['face']) & (a['face'] >= 0)
    err = np.abs(a['color'] - b['color'].astype(np.float64))[agree]
    print('%dx%d: covered %.3f, float32 vs float64 face id differs on %.2e of the pixels; colour error on agreeing pixels max %.2e median %.2e'
          % (H, W, (a['face'] >= 0).mean(), differ, err.max(), np.median(err)))
    assert (a['face'] >= 0).mean() > 0.02
    assert differ < 1e-3
    # all three persons are in the picture, two of them overlap, one is cut by the border
    F = f.shape[0]
    assert set(np.unique(a['face'][a['face'] >= 0] // F)) == {0, 1, 2}
    assert (a['face'][:, -1] >= 0).any()


def test_renderer_refuses_cpu_tensors():
    from whmr_amd.utils.renderer_cam import MeshRenderer, vertex_face_csr
    v, f = MR.uv_sphere()
    r = MeshRenderer(f)
    ptr, idx = vertex_face_csr(f, 6890)
    assert ptr[-1] == 3 * 13776 and (np.diff(ptr) >= 4).all()
    for k in (0, 100, 6889):
        assert all(k in f[j] for j in idx[ptr[k]:ptr[k + 1]]) and (np.diff(idx[ptr[k]:ptr[k + 1]]) > 0).all()
    with pytest.raises(RuntimeError):
        r.render(torch.zeros(64, 64, 3, dtype=torch.uint8), torch.from_numpy(v).float()[None], torch.tensor([[0.0, 0.0, 3.0]]), torch.tensor([500.0]))
    with pytest.raises(ValueError):
        MeshRenderer(np.array([[0, 1, -2]]))
