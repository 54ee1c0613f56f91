"""Host side of the ground plane of the mesh renderer (whmr_mesh_render_scene: MeshRenderer.plan_grounds, _lib.RENDER_GROUND_DTYPE, the ``ground``
arguments) and of ``export_obj``; and the plane's float64 restatement (tests/mesh_ground_reference.py) against answers worked out by hand and against
itself in float32."""
import os
import re

import numpy as np
import pytest
import torch

import mesh_ground_reference as MG
import mesh_render_reference as MR
from conftest import ROOT
from whmr_amd import _lib as L
from whmr_amd.utils import renderer_cam as RC
from whmr_amd.utils.renderer_cam import MeshRenderer

FACES = MR.uv_sphere(rings=6, segments=7)[1]          # 84 faces, 44 vertices


def test_ground_row_has_the_layout_the_kernel_file_asserts():
    text = open(os.path.join(ROOT, 'w-hmr_amd', 'csrc', 'mesh_render.hip')).read()
    sizes = {k: int(v) for k, v in re.findall(r'static_assert\(sizeof\((whmr_ground_\w+)\) == (\d+),', text)}
    assert sizes == {'whmr_ground_row': 32}
    fields = {f: int(off) for f, off in re.findall(r'static_assert\(offsetof\(whmr_ground_row, (\w+)\) == (\d+),', text)}
    dtype = L.RENDER_GROUND_DTYPE
    assert dtype.itemsize == 32 and list(dtype.names) == list(fields)                     # every field asserted, in the record's order
    assert {n: dtype.fields[n][1] for n in dtype.names} == fields
    body = re.search(r'struct whmr_ground_row \{(.*?)\n\};', text, flags=re.S).group(1)
    body = re.sub(r'//[^\n]*', '', body)
    declared = [re.search(r'(\w+)\s*(?:\[[^\]]*\])?\s*$', p).group(1) for decl in body.split(';') for p in decl.split(',') if p.strip()]
    assert declared == list(dtype.names)                                                  # and no field of the struct left out of the asserts
    kinds = {n: dtype.fields[n][0].str for n in dtype.names}
    assert kinds == dict(draw='<i4', given='<i4', y='<f4', half='<f4', n='<i4', dark='<f4', light='<f4', reserved='<i4')
    assert 'whmr_mesh_render_scene' in L.EXPORTS


def test_plan_grounds_values():
    r = MeshRenderer(FACES, ground_colors=(0.25, 0.75))
    assert MeshRenderer(FACES).ground_colors == (35 / 255, 220 / 255) and r.color == RC.DEFAULT_COLOR
    # four images: a strip's frame (no draw), its overlay, and two side views
    draws = [(0, 0, 1, 0), (0, 0, 2, 270), (0, 1, 3, 270)]
    g = r.plan_grounds(4, draws, [(2, 1, None), (3, 2, -0.5, 1.5, 4)])
    assert g.dtype == L.RENDER_GROUND_DTYPE and g.shape == (4,)
    assert g['draw'].tolist() == [-1, -1, 1, 2] and g['given'].tolist() == [0, 0, 0, 1]
    assert g['y'].tolist() == [0.0, 0.0, 0.0, -0.5] and g['half'][2:].tolist() == [2.0, 1.5] and g['n'][2:].tolist() == [9, 4]
    assert g['dark'][2:].tolist() == [0.25, 0.25] and g['light'][2:].tolist() == [0.75, 0.75] and not g['reserved'].any()
    raw = g.view(np.uint8).reshape(4, 32)                                                 # the bytes that go up: fields where the header says
    assert raw[3, :8].view('<i4').tolist() == [2, 1] and raw[3, 8:16].view('<f4').tolist() == [-0.5, 1.5] and raw[3, 16:20].view('<i4').tolist() == [4]
    assert raw[3, 20:28].view('<f4').tolist() == [0.25, 0.75] and raw[0, :4].view('<i4').tolist() == [-1]
    # no plane at all is a table too, and plan_draws still returns its three values
    assert r.plan_grounds(2, draws[:1], [])['draw'].tolist() == [-1, -1]
    assert len(r.plan_draws([(8, 8)] * 4, draws, have_verts1=True)) == 3
    # a height of 0.0 is a height, not "off"
    assert r.plan_grounds(2, draws[:1], [(1, 0, 0.0)])['given'].tolist() == [0, 1]


def test_plan_grounds_value_errors():
    r = MeshRenderer(FACES)
    draws = [(0, 0, 0, 0), (1, 0, 1, 0), (2, 0, 1, 0), (3, 0, 2, 270)]                   # image 1 is shared by draws 1 and 2
    with pytest.raises(ValueError, match='two ground planes'):
        r.plan_grounds(3, draws, [(0, 0, None), (0, 0, -1.0)])
    with pytest.raises(ValueError, match='targets image'):
        r.plan_grounds(3, draws, [(2, 0, None)])                                          # draw 0 draws into image 0
    with pytest.raises(ValueError, match='shared by 2 draws'):
        r.plan_grounds(3, draws, [(1, 1, None)])
    for bad in (4, -1):
        with pytest.raises(ValueError, match='names draw'):
            r.plan_grounds(3, draws, [(0, bad, None)])
    for bad in (3, -1):
        with pytest.raises(ValueError, match='names image'):
            r.plan_grounds(3, draws, [(bad, 0, None)])
    for half, n in ((2.0, 0), (0.0, 9), (-1.0, 9), (float('nan'), 9)):
        with pytest.raises(ValueError, match='tiles per side'):
            r.plan_grounds(3, draws, [(0, 0, None, half, n)])
    with pytest.raises(ValueError, match='tiles per side'):
        r.plan_grounds(3, draws, [(0, 0, None)], n=0)
    assert r.plan_grounds(3, draws, [(0, 0, None), (2, 3, 1.0)])['draw'].tolist() == [0, -1, 3]


class _OnDevice(torch.Tensor):
    """a host tensor that answers ``is_cuda`` like a device one"""
    is_cuda = property(lambda self: True)


def test_a_plane_on_a_shared_image_is_refused_before_anything_is_launched(monkeypatch):
    from whmr_amd import demo

    def no_launch(*a, **k):
        raise AssertionError('nothing may be launched')
    monkeypatch.setattr(L, 'lib', no_launch)
    r = MeshRenderer(FACES)
    dev = lambda t: t.as_subclass(_OnDevice)
    frame, frames = dev(torch.zeros(8, 8, 3, dtype=torch.uint8)), dev(torch.zeros(2, 8, 8, 3, dtype=torch.uint8))
    verts, cam_t, focal = dev(torch.zeros(2, 44, 3)), dev(torch.zeros(2, 3)), dev(torch.ones(2))
    for ground in (True, 0.0, -0.7):
        with pytest.raises(ValueError, match='ground plane'):
            r.render(frame, verts, cam_t, focal, ground=ground)
        with pytest.raises(ValueError, match='ground plane'):
            r.render_clip(frames, verts, cam_t, focal, [0, 0], ground=ground)
        with pytest.raises(ValueError, match='ground plane'):
            demo.render_frame(dict(local_smpl_vertices=verts, pred_cam_t=cam_t, focal_length=focal), frame, r, ground=ground)


def test_plane_by_hand():
    """R = I, t = 0, h = -1, f = 40, centre (cx, cy) = (24, 16), an image 32 wide and 48 high: the camera stands at the origin, one metre above the
    plane, looking along world -z.  Row j <= 15 looks up: no plane.  Row j >= 16 meets it at Z_g = 40 / (j + 0.5 - 16), in the point
    q = (Z_g a, -1, -Z_g) with a = (i + 0.5 - 24) / 40; the square ends at q_z = -2, so only Z_g <= 2 lies on it: rows j >= 36 (40 / 20.5 = 1.95),
    which is why the image has to be the 48 high.  Tiles: side 4 / 9 = 0.4444."""
    cov, Z, ix, iz = MG.plane(48, 32, (0, 0, 0), (40, 40), (24, 16), None, -1.0)
    assert not cov[:36].any() and cov[36:].all()                                          # |q_x| <= 2 * 23.5 / 40 everywhere: no column leaves the square
    for j in range(16, 48):
        assert np.allclose(Z[j], 40 / (j + 0.5 - 16), rtol=1e-14)
    # pixel (j, i) = (36, 24): Z_g = 1.95122, q_x = 1.95122 * 0.5 / 40 = 0.02439, q_z = -1.95122
    #   ix = floor(2.02439 / 0.44444) = floor(4.555) = 4, iz = floor(0.04878 / 0.44444) = 0
    # pixel (47, 24): Z_g = 40 / 31.5 = 1.26984, q_x = 0.01587, q_z = -1.26984:  ix = floor(4.536) = 4, iz = floor(0.73016 / 0.44444) = floor(1.643) = 1
    # pixel (40, 0): Z_g = 40 / 24.5 = 1.63265, a = -23.5 / 40, q_x = -0.95918, q_z = -1.63265:  ix = floor(1.04082 / 0.44444) = floor(2.342) = 2,
    #   iz = floor(0.36735 / 0.44444) = 0
    # pixel (47, 31): a = 7.5 / 40, q_x = 0.23810: ix = floor(2.23810 / 0.44444) = floor(5.036) = 5, iz = 1
    assert (ix[36, 24], iz[36, 24]) == (4, 0) and (ix[47, 24], iz[47, 24]) == (4, 1) and (ix[40, 0], iz[40, 0]) == (2, 0) and (ix[47, 31], iz[47, 31]) == (5, 1)
    assert not cov[35, 24] and Z[35, 24] > 2                                              # 40 / 19.5 = 2.05: the plane's height is met beyond the square
    # The same camera half a metre above the plane (given h = -0.5), through the whole restatement: Z_g = 20 / (j + 0.5 - 16).
    # pixel (39, 24): Z_g = 0.85106, q_z = -0.85106, iz = floor(1.14894 / 0.44444) = floor(2.585) = 2, ix = floor(2.01064 / 0.44444) = 4: tile 38, dark
    # pixel (33, 24): Z_g = 20 / 17.5 = 1.14286, iz = floor(0.85714 / 0.44444) = floor(1.929) = 1, ix = 4: tile 37, 4 + 1 odd: light
    frame = np.full((48, 32, 3), 9, np.uint8)
    tri = np.array([[[0.0, 0.0, 5.0], [0.01, 0.0, 5.0], [0.0, 0.01, 5.0]]])            # a speck of a mesh, far behind where the rays meet the plane
    faces = np.array([[0, 1, 2]], np.int32)
    out = MG.render(frame, tri, faces, np.zeros((1, 3)), np.full(1, 40.0), center=(24, 16), ground=-0.5)
    assert out['ground'][0, 39, 24] == 38 and (out['image'][0, 39, 24] == 35).all() and out['face'][0, 39, 24] == -1
    assert out['ground'][0, 33, 24] == 37 and (out['image'][0, 33, 24] == 220).all()
    assert abs(out['depth'][0, 39, 24] - 20 / 23.5) < 1e-12 and out['ground_y'].tolist() == [-0.5]
    assert (out['ground'][0, :16] == -1).all() and (out['image'][0, :15] == 9).all()      # above the horizon: the frame's bytes
    # without a given height the plane hangs from the mesh's lowest point: world y = -p_y, and the speck's largest p_y is 0.01
    assert MG.render(frame, tri, faces, np.zeros((1, 3)), np.full(1, 40.0), center=(24, 16))['ground_y'].tolist() == [-0.01]
    assert np.isnan(MG.lowest_point(np.full((1, 3, 3), np.nan))).all() and MG.lowest_point(np.array([[[0, np.nan, 0], [0, 0.25, 0]]])).tolist() == [-0.25]


@pytest.mark.parametrize('size,angle,tilted', MG.SCENES)
def test_reference_in_float32_against_itself_in_float64(size, angle, tilted):
    """what single precision alone changes on the scenes of the GPU test: the class of a pixel (face id / tile / background) on less than 2e-3 of the
    pixels, the cap tests/test_mesh_render_gpu.py gives fp32-against-float64 edge decisions.  Measured: 0 on all eight scenes; plane depth on agreeing
    pixels differs by at most 8.9e-7."""
    H, W = size
    scene, ref = MG.scene_reference(size, angle, tilted)
    f32 = MG.render(np.zeros((H, W, 3), np.uint8), scene['verts'], scene['faces'], scene['cam_t'], scene['focal'], rot=scene['rot'], sideview_angle=angle,
                    dtype=np.float32)
    c64, c32 = MG.pixel_class(ref['face'], ref['ground']), MG.pixel_class(f32['face'], f32['ground'])
    on_plane = (c64 == c32) & (ref['ground'] >= 0)
    differ, derr = (c64 != c32).mean(), np.abs(f32['depth'] - ref['depth'])[on_plane].max()
    print('%dx%d angle %d tilted %s: class differs on %.2e of the pixels; plane on %.3f; plane depth error %.2e' % (H, W, angle, tilted, differ,
                                                                                                                 (ref['ground'] >= 0).mean(), derr))
    assert (ref['ground'] >= 0).mean() > 0.1 and (ref['face'] >= 0).mean() > 0.02
    assert differ < 2e-3 and derr < 1e-4
    assert np.array_equal(f32['ground_y'].astype(np.float64), ref['ground_y'])            # a maximum of float32 numbers: exact in both


def _parse_obj(path):
    v, f = [], []
    for line in open(path):
        kind, *rest = line.split()
        (v if kind == 'v' else f).append(rest)
        assert kind in ('v', 'f') and len(rest) == 3
    return np.array(v, dtype=np.float64).astype(np.float32), np.array(f, dtype=np.int64)


def test_export_obj(tmp_path):
    rng = np.random.default_rng(5)
    verts = rng.standard_normal((44, 3)).astype(np.float32)
    t = np.array([0.25, -0.5, 3.0], np.float32)
    path = str(tmp_path / 'person.obj')
    RC.export_obj(path, torch.from_numpy(verts), FACES, camera_translation=torch.from_numpy(t))
    v, f = _parse_obj(path)
    assert np.array_equal(v, (verts.astype(np.float64) * [1, -1, -1]).astype(np.float32)) and np.array_equal(f, FACES + 1)
    assert np.array_equal(np.load(str(tmp_path / 'person.npy')), np.array([-0.25, -0.5, 3.0], np.float32))
    assert open(path).readline() == 'v %.9g %.9g %.9g\n' % tuple(float(x) for x in v[0])
    # a side view: the vertices after D and S; a _rot.obj carries no camera file
    rot = str(tmp_path / 'person_rot.obj')
    RC.export_obj(rot, verts, torch.from_numpy(FACES), sideview_angle=270)
    v, f = _parse_obj(rot)
    assert np.array_equal(v, (verts.astype(np.float64) @ MR.world_matrix(270).T).astype(np.float32)) and np.array_equal(f, FACES + 1)
    assert sorted(os.listdir(tmp_path)) == ['person.npy', 'person.obj', 'person_rot.obj']
    assert np.array_equal(torch.from_numpy(t).numpy(), [0.25, -0.5, 3.0])                 # the caller's translation is not modified
    with pytest.raises(ValueError, match='camera translation'):
        RC.export_obj(str(tmp_path / 'other.obj'), verts, FACES)
