"""Host side of the draw-list renderer (whmr_amd.utils.renderer_cam.MeshRenderer.plan_draws / render_clip, whmr_amd._lib.RENDER_*_DTYPE): the two
tables of whmr_mesh_render_draws as the host packs them, against the layout that csrc/mesh_render.hip asserts at compile time, and every error
that has to come before a launch."""
import math
import os
import re

import numpy as np
import pytest
import torch

import mesh_render_reference as MR
from conftest import ROOT
from whmr_amd import _lib as L
from whmr_amd.utils.renderer_cam import MeshRenderer

FACES = MR.uv_sphere(rings=6, segments=7)[1]          # 84 faces


def _asserted_layout():
    """{struct: ({field: offset}, size)} from the static_asserts of the kernel file: the C side of the table layout, checked by the compiler"""
    text = open(os.path.join(ROOT, 'w-hmr_amd', 'csrc', 'mesh_render.hip')).read()
    sizes = {k: int(v) for k, v in re.findall(r'static_assert\(sizeof\((whmr_render_\w+)\) == (\d+),', text)}
    fields = {k: {} for k in sizes}
    for k, f, off in re.findall(r'static_assert\(offsetof\((whmr_render_\w+), (\w+)\) == (\d+),', text):
        fields[k][f] = int(off)
    return {k: (fields[k], sizes[k]) for k in sizes}, text


def test_table_records_have_the_layout_the_kernel_file_asserts():
    layout, text = _asserted_layout()
    assert set(layout) == {'whmr_render_image', 'whmr_render_draw'}
    for cname, dtype in (('whmr_render_image', L.RENDER_IMAGE_DTYPE), ('whmr_render_draw', L.RENDER_DRAW_DTYPE)):
        fields, size = layout[cname]
        assert dtype.itemsize == size and list(dtype.names) == list(fields)               # every field asserted, in the record's order
        assert {n: dtype.fields[n][1] for n in dtype.names} == fields
        body = re.search(r'struct %s \{(.*?)\n\};' % cname, text, flags=re.S).group(1)
        body = re.sub(r'//[^\n]*', '', body)
        declared = [re.search(r'(\w+)\s*(?:\[[^\]]*\])?\s*$', p).group(1) for decl in body.split(';') for p in decl.split(',') if p.strip()]
        assert declared == list(dtype.names), cname                                      # and no field of the struct left out of the asserts
    kinds = {n: L.RENDER_IMAGE_DTYPE.fields[n][0].str for n in L.RENDER_IMAGE_DTYPE.names}
    assert kinds == dict(frame='<u8', out='<u8', frame_row_stride='<i8', out_row_stride='<i8', pix_off='<i8', H='<i4', W='<i4', cx='<f4', cy='<f4')
    kinds = {n: L.RENDER_DRAW_DTYPE.fields[n][0].base.str for n in L.RENDER_DRAW_DTYPE.names}
    assert kinds == dict(row='<i4', verts_set='<i4', image='<i4', side_cos='<f4', side_sin='<f4', reserved='<i4')
    assert 'whmr_mesh_render_draws' in L.EXPORTS


def test_plan_draws_three_images_four_draws():
    r = MeshRenderer(FACES)
    sizes = [(48, 64), (40, 56), (33, 47)]
    # image 2 is a panel of a strip [33, 4 * 47, 3]; image 1's background is a row-strided view of a wider frame
    draws = [(0, 0, 0, 0), (1, 0, 0, 0), (3, 1, 2, 270), (2, 0, 1, 90)]
    images, table, total = r.plan_draws(sizes, draws, centers=[(32, 24), (28.5, 20.25), (23, 16)], frame_strides=[192, 3 * 80, 141],
                                        out_strides=[192, 168, 4 * 141], have_verts1=True, n_rows=4)
    assert images.dtype == L.RENDER_IMAGE_DTYPE and table.dtype == L.RENDER_DRAW_DTYPE and images.shape == (3,) and table.shape == (4,)
    assert images['H'].tolist() == [48, 40, 33] and images['W'].tolist() == [64, 56, 47]
    assert images['pix_off'].tolist() == [0, 48 * 64, 48 * 64 + 40 * 56] and total == 48 * 64 + 40 * 56 + 33 * 47
    assert images['cx'].tolist() == [32.0, 28.5, 23.0] and images['cy'].tolist() == [24.0, 20.25, 16.0]
    assert images['frame_row_stride'].tolist() == [192, 240, 141] and images['out_row_stride'].tolist() == [192, 168, 564]
    assert not images['frame'].any() and not images['out'].any()                          # the pointers are the caller's
    assert table['row'].tolist() == [0, 1, 3, 2] and table['verts_set'].tolist() == [0, 0, 1, 0] and table['image'].tolist() == [0, 0, 2, 1]
    f32 = lambda v: float(np.float32(v))
    assert table['side_cos'].tolist() == [1.0, 1.0, f32(math.cos(math.radians(270.0))), f32(math.cos(math.radians(90.0)))]
    assert table['side_sin'].tolist() == [0.0, 0.0, f32(math.sin(math.radians(270.0))), f32(math.sin(math.radians(90.0)))]
    assert not table['reserved'].any()
    # the bytes that go up: rows of 56 and 32 bytes, fields where the header says
    raw = images.view(np.uint8).reshape(3, 56)
    assert raw[2, 32:40].view('<i8')[0] == 48 * 64 + 40 * 56 and raw[2, 40:48].view('<i4').tolist() == [33, 47] and raw[1, 48:56].view('<f4').tolist() == [28.5, 20.25]
    assert table.view(np.uint8).reshape(4, 32)[2, :12].view('<i4').tolist() == [3, 1, 2]
    # defaults: the frame centre (W // 2, H // 2), packed rows
    images, table, total = r.plan_draws(sizes, [(0, 0, 1, 0)])
    assert images['cx'].tolist() == [32.0, 28.0, 23.0] and images['cy'].tolist() == [24.0, 20.0, 16.0]
    assert images['frame_row_stride'].tolist() == images['out_row_stride'].tolist() == [192, 168, 141]
    # no draw at all is a plan too (every image is its background)
    assert r.plan_draws(sizes, [])[1].shape == (0,)


def test_plan_draws_value_errors():
    r = MeshRenderer(FACES)
    sizes = [(48, 64), (40, 56)]
    for bad in (2, -1):
        with pytest.raises(ValueError, match='image'):
            r.plan_draws(sizes, [(0, 0, 0, 0), (0, 0, bad, 0)])
    for bad in ([(48, 0)], [(0, 64)], [(48, 64), (-1, 3)], []):
        with pytest.raises(ValueError, match='image'):
            r.plan_draws(bad, [])
    with pytest.raises(ValueError, match='verts_set'):
        r.plan_draws(sizes, [(0, 1, 0, 0)])                                              # no second vertex tensor
    with pytest.raises(ValueError, match='verts_set'):
        r.plan_draws(sizes, [(0, 2, 0, 0)], have_verts1=True)
    assert r.plan_draws(sizes, [(0, 1, 0, 0)], have_verts1=True)[1]['verts_set'].tolist() == [1]
    with pytest.raises(ValueError, match='row'):
        r.plan_draws(sizes, [(3, 0, 0, 0)], n_rows=3)
    with pytest.raises(ValueError, match='row'):
        r.plan_draws(sizes, [(-1, 0, 0, 0)])

    class Many(list):                                                                    # D * F >= 2^31 without building 25 million draws
        def __len__(self):
            return -(-2 ** 31 // 84)
    with pytest.raises(ValueError, match='2\\^31'):
        r.plan_draws(sizes, Many())
    assert (-(-2 ** 31 // 84) - 1) * 84 < 2 ** 31                                        # one draw fewer would pass


class _OnDevice(torch.Tensor):
    """a host tensor that answers ``is_cuda`` like a device one"""
    is_cuda = property(lambda self: True)


def test_render_clip_refuses_a_device_frame_index_and_host_tensors(monkeypatch):
    from whmr_amd.utils.renderer_cam import render_clip_groups

    def no_launch(*a, **k):
        raise AssertionError('nothing may be launched')
    monkeypatch.setattr(L, 'lib', no_launch)
    r = MeshRenderer(FACES)
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    verts, cam_t, focal = torch.zeros(2, 44, 3), torch.zeros(2, 3), torch.ones(2)
    on_device = torch.zeros(2, dtype=torch.int64).as_subclass(_OnDevice)
    with pytest.raises(RuntimeError, match='frame_index'):
        r.render_clip(frames, verts, cam_t, focal, on_device)
    with pytest.raises(RuntimeError, match='frame_index'):
        render_clip_groups(frames, cam_t, verts, verts, None, focal, on_device, r)
    with pytest.raises(RuntimeError, match='no CPU fallback'):                           # host frames: no CPU path
        r.render_clip(frames, verts, cam_t, focal, [0, 1])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        render_clip_groups(frames, cam_t, verts, verts, None, focal, [0, 1], r)
