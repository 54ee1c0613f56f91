"""Host side of the marked form of the mesh renderer (whmr_mesh_render_marked: keypoint skeletons and wireframe): the two table layouts against the
static_asserts of csrc/mesh_render.hip, the planners and their ValueErrors, the skeleton constants against the fixture written from the reference's
kp_utils.py, and self-checks of the float64 restatement (tests/mesh_marks_reference.py).  No GPU."""
import os
import re

import numpy as np
import pytest

import mesh_marks_reference as MM
from conftest import ROOT
from whmr_amd import _lib as L
from whmr_amd.core import constants as K
from whmr_amd.utils.renderer_cam import MeshRenderer

TRI = np.array([[0, 1, 2]])


def _asserted_layout(struct):
    """{field: offset} and the size of ``struct`` from the static_asserts of the kernel file"""
    src = open(os.path.join(ROOT, 'w-hmr_amd', 'csrc', 'mesh_render.hip')).read()
    size = int(re.search(r'static_assert\(sizeof\(%s\) == (\d+)' % struct, src).group(1))
    return {f: int(o) for f, o in re.findall(r'static_assert\(offsetof\(%s, (\w+)\) == (\d+)' % struct, src)}, size


@pytest.mark.parametrize('struct,dtype', [('whmr_style_row', L.RENDER_STYLE_DTYPE), ('whmr_skeleton_row', L.RENDER_SKELETON_DTYPE)])
def test_table_rows_have_the_layout_the_kernel_file_asserts(struct, dtype):
    offsets, size = _asserted_layout(struct)
    assert size == dtype.itemsize and len(offsets) >= 3
    # every field of the struct is asserted, and every asserted field is a field of the dtype at that offset (side_cos, side_sin / half_width, radius
    # are declared two to a line: the dtype names them one by one)
    src = open(os.path.join(ROOT, 'w-hmr_amd', 'csrc', 'mesh_render.hip')).read()
    body = re.search(r'struct %s \{(.*?)\};' % struct, src, flags=re.S).group(1)
    declared = [n for line in re.sub(r'//[^\n]*', '', body).split(';') for n in re.findall(r'(\w+)(?:\[\d+\])?\s*(?:,|$)', line.strip())]
    assert declared == list(dtype.names) == list(offsets)
    assert {n: dtype.fields[n][1] for n in dtype.names} == offsets
    assert all(dtype.fields[n][0].base.itemsize == 4 and dtype.fields[n][0].base.byteorder in '<=' for n in dtype.names)      # int32 / float, little-endian


def test_bin_capacity_is_one_number_on_all_three_sides():
    src = open(os.path.join(ROOT, 'w-hmr_amd', 'csrc', 'mesh_render.hip')).read()
    hdr = open(os.path.join(ROOT, 'include', 'whmr_hip.h')).read()
    assert int(re.search(r'#define MESH_BIN_SKELETONS (\d+)', src).group(1)) == L.MESH_BIN_SKELETONS
    assert int(re.search(r'#define WHMR_MESH_BIN_SKELETONS (\d+)', hdr).group(1)) == L.MESH_BIN_SKELETONS


def test_plan_styles():
    r = MeshRenderer(TRI)
    t = r.plan_styles(3)
    assert t.dtype == L.RENDER_STYLE_DTYPE and t['mode'].tolist() == [0, 0, 0] and not t['reserved'].any()
    t = r.plan_styles(3, wireframe=True, line_width=3.0)
    assert t['mode'].tolist() == [1, 1, 1] and t['half_width'].tolist() == [1.5, 1.5, 1.5]
    t = r.plan_styles(2, wireframe=[True, False], line_width=[1.0, 4.0])
    assert t['mode'].tolist() == [1, 0] and t['half_width'].tolist() == [0.5, 2.0]
    assert r.plan_styles(1, True)['half_width'][0] == np.float32(0.5 * K.WIREFRAME_LINE_WIDTH)
    assert len(r.plan_styles(0)) == 0
    for bad in (dict(wireframe=[True]), dict(line_width=[1.0]), dict(line_width=-1.0), dict(line_width=float('nan')), dict(line_width=float('inf'))):
        with pytest.raises(ValueError):
            r.plan_styles(2, **bad)


def test_plan_skeletons():
    r = MeshRenderer(TRI)
    t = r.plan_skeletons(2, [(0, 1, 0, 'over', 270), (3, 0, 1, 'under', 0, 5.0, 2.0), (1, 1, 0, 1, 90)], n_rows=4)
    assert t.dtype == L.RENDER_SKELETON_DTYPE
    assert t['row'].tolist() == [0, 3, 1] and t['image'].tolist() == [1, 0, 1] and t['source'].tolist() == [0, 1, 0] and t['layer'].tolist() == [1, 0, 1]
    assert np.allclose(t['side_cos'], [0, 1, 0], atol=1e-6) and np.allclose(t['side_sin'], [-1, 0, 1], atol=1e-6)
    assert t['half_width'].tolist() == [np.float32(0.5 * K.SKELETON_BONE_WIDTH), 2.5, np.float32(0.5 * K.SKELETON_BONE_WIDTH)]
    assert t['radius'].tolist() == [np.float32(K.SKELETON_JOINT_RADIUS), 2.0, np.float32(K.SKELETON_JOINT_RADIUS)]
    assert r.plan_skeletons(1, [(0, 0, 0, 0, 0)], bone_width=4.0, joint_radius=0.0)[0].tolist()[6:] == (2.0, 0.0)
    assert len(r.plan_skeletons(1, [])) == 0
    for bad in ((4, 0, 0, 'under', 0), (-1, 0, 0, 'under', 0), (0, 2, 0, 'under', 0), (0, -1, 0, 'under', 0), (0, 0, 2, 'under', 0), (0, 0, 0, 'above', 0),
                (0, 0, 0, 2, 0), (0, 0, 0, 'under', 0, -1.0, 1.0), (0, 0, 0, 'under', 0, 1.0, float('nan'))):
        with pytest.raises(ValueError):
            r.plan_skeletons(2, [bad], n_rows=4)


def test_renderer_skeleton_arguments():
    r = MeshRenderer(TRI)
    assert r.bones.tolist() == [list(b) for b in K.SPIN_SKELETON] and r.n_joints_min == 39
    assert r.bone_colors.shape == (25, 3) and [tuple(c) for c in r.bone_colors.tolist()] == [tuple(np.float32(K.SKELETON_SIDE_RGB[s]).tolist())
                                                                                             for s in K.SPIN_BONE_SIDE]
    own = MeshRenderer(TRI, skeleton=[(0, 1), (1, 2)], bone_colors=[(1, 0, 0), (0, 1, 0)], joint_color=(0, 0, 1))
    assert own.bones.tolist() == [[0, 1], [1, 2]] and own.n_joints_min == 3
    assert MeshRenderer(TRI, skeleton=[(0, 1)]).bone_colors.tolist() == [list(np.float32(K.SKELETON_SIDE_RGB['c']).tolist())]
    for bad in (dict(skeleton=[(0, -1)]), dict(skeleton=[(0, 1)], bone_colors=[(1, 0, 0)] * 2), dict(bone_colors=[(2.0, 0, 0)] * 25), dict(joint_color=(1, 1))):
        with pytest.raises(ValueError):
            MeshRenderer(TRI, **bad)


def _side(name):
    """'l' / 'r' / 'c' of a name of get_spin_joint_names(): 'OP LKnee', 'OP RHeel', 'lankle', 'rear' (the right ear) ...; 'OP Neck', 'headtop' are centre"""
    if name.startswith('OP '):
        return name[3].lower() if name[3] in 'LR' and name[4].isupper() else 'c'
    return name[0] if name[0] in 'lr' and name[1:] in ('ankle', 'knee', 'hip', 'wrist', 'elbow', 'shoulder', 'eye', 'ear') else 'c'


def test_skeleton_constants_against_the_reference_fixture():
    """tests/golden/skeleton.npz: get_spin_skeleton() and get_spin_joint_names() of the reference's kp_utils.py (make_golden_skeleton.py)"""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'skeleton.npz'))
    bones, names = g['bones'], g['names'].tolist()
    assert bones.shape == (25, 2) and len(names) == 49 == len(K.JOINT_MAP_49)
    assert [tuple(b) for b in bones.tolist()] == K.SPIN_SKELETON
    assert names[8] == 'OP MidHip' and names[38] == 'headtop' and names[48] == 'rear'
    sides = []
    for a, b in bones.tolist():
        s = {_side(names[a]), _side(names[b])} - {'c'}
        assert len(s) <= 1                                                      # no bone joins a left joint to a right one
        sides.append(s.pop() if s else 'c')
    assert ''.join(sides) == K.SPIN_BONE_SIDE and set(K.SKELETON_SIDE_RGB) == {'l', 'r', 'c'}
    assert sides.count('l') == sides.count('r') == 11 and sides.count('c') == 3


# ---- the restatement, on its own
@pytest.mark.parametrize('half_width', [0.5, 1.0, 2.25])
def test_a_horizontal_bones_coverage_sums_to_its_area(half_width):
    """a bone from (10.3, 20.4) to (50.3, 20.4): the ramp clamp(h + 0.5 - d, 0, 1) integrates across the line to 2 h exactly when it is sampled at
    the pixel centres (spacing 1: the ramps of the two sides are sampled at offsets that add up), so the body gives 2 h per column; the two end caps
    are half discs of the same ramp, integral pi (h^2 + 1/4) together, sampled at ~pi h^2 centres: midpoint rule, error below the cap's perimeter
    2 pi (h + 0.5) times the largest sampling error per boundary pixel, 1/4"""
    length = 40.0
    cov = MM.cover(48, 64, np.array([10.3, 20.4]), np.array([50.3, 20.4]), half_width + 0.5)
    assert cov.min() >= 0 and cov.max() <= 1
    want = 2 * half_width * length + np.pi * (half_width ** 2 + 0.25)
    assert abs(cov.sum() - want) < 2 * np.pi * (half_width + 0.5) * 0.25, (cov.sum(), want)
    col = cov[:, 30]                                                            # a column through the body: exactly 2 h
    assert abs(col.sum() - 2 * half_width) < 1e-12
    dot = MM.cover(48, 64, np.array([30.5, 20.5]), np.array([30.5, 20.5]), 3.5)     # a bone without length is a dot
    assert dot[20, 30] == 1 and dot[20, 34] == 0 and abs(dot[20, 33] - 0.5) < 1e-12


def test_wire_alpha_is_one_on_an_edge_and_zero_at_the_incentre():
    scr = np.array([[10.0, 10.0, 1.0], [50.5, 12.0, 1.0], [22.0, 44.5, 1.0]])
    faces = np.array([[0, 1, 2]])
    fid = np.zeros((48, 64), np.int64)                                          # every pixel asks about face 0
    a = MM.wire_alpha(fid, scr, faces, 0.75)
    # the incentre: the in-circle's radius is far beyond the line
    p = scr[:, :2]
    l = np.array([np.linalg.norm(p[1] - p[2]), np.linalg.norm(p[2] - p[0]), np.linalg.norm(p[0] - p[1])])
    inc = (l[:, None] * p).sum(0) / l.sum()
    assert a[int(inc[1]), int(inc[0])] == 0
    # pixel centres within 1/4 pixel of the edge 0 -> 1: alpha 1 (half_width + 0.5 - d >= 1)
    px, py = np.meshgrid(np.arange(64) + 0.5, np.arange(48) + 0.5)
    d01 = np.abs((px - p[0, 0]) * (p[1, 1] - p[0, 1]) - (py - p[0, 1]) * (p[1, 0] - p[0, 0])) / l[2]
    near = d01 <= 0.25
    assert near.sum() > 5 and (a[near] == 1).all()
    assert ((a > 0) & (a < 1)).sum() > 20 and (MM.wire_alpha(np.full((48, 64), -1), scr, faces, 0.75) == 0).all()
    assert (MM.wire_alpha(fid, scr, faces, 1e4) == 1).all()                      # a line wider than the face: solid


def test_keypoint_validity():
    kp = MM.keypoints(np.array([[0, 0, 0], [0, 0, -2.0], [np.nan, 0, 0], [0.1, 0.2, 0.3]]), [0.0, 0.0, 1.0], [100.0, 100.0], (32, 24))
    assert kp[0].tolist() == [32.0, 24.0, 1.0] and kp[1, 2] == 0 and kp[2, 2] == 0 and kp[3, 2] == 1.3       # depth -1 is behind znear
    g = MM.given_keypoints(np.array([[1, 2, 0.5], [1, np.inf, 1], [3, 4, -1.0], [np.nan, 0, 1]]))
    assert g[:, 2].tolist() == [0.5, 0, -1.0, 0]


def test_the_gpu_scene_is_not_vacuous():
    """the asserts tests/test_mesh_marks_gpu.py makes about its scene, on the restatement alone"""
    r = MeshRenderer(TRI)
    jr = np.broadcast_to(r.joint_color, (49, 3))
    for tilted in (False, True):
        sc, refs, kps = MM.scene_reference(tilted, r.bones, r.bone_colors, jr)
        assert MM.non_vacuous(sc, refs, kps)
