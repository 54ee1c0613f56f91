"""Clip inference on the device: whmr_resize_normalize_frames against the Pillow fixture (tests/golden/frames.npz) and the restatement pinned to it
(tests/frames_reference.py), whmr_crop_normalize_frames against the per-frame kernel, WHMR.forward(frame_index=...), infer_clip and ClipPipeline
against the per-frame path."""
import os

import numpy as np
import pytest
import torch

import frames_reference as FR
from conftest import GOLDEN, ew_err
from test_clip_cpu import CASES, ONE_AXIS

pytestmark = pytest.mark.gpu
GATE = 1e-4                                          # the project's element-wise parity gate (tests/test_hotpath_gpu.py)


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(GOLDEN, 'frames.npz')))


@pytest.fixture(scope='module')
def model(dev, assets, state_dict):
    from whmr_amd.models import whmr_net
    m = whmr_net(None, assets=assets, numerics='fp32')
    m.load_state_dict(state_dict, strict=False)
    return m.to(dev).eval()


def _normalised_by_torch(u8, dev):
    """(u8.float() / 255 - mean) / std by torch on the device, NCHW.  255 is a device tensor: torch's HIP division by a HOST scalar multiplies by
    the rounded reciprocal (one unit in the last place off for 180 of the 256 byte values), while ToTensor on the reference's CPU divides."""
    from whmr_amd.datasets.img_utils import MEAN, STD
    mean, std = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1), torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    return (u8.permute(0, 3, 1, 2).float() / torch.tensor(255., device=dev) - mean) / std


def _check_resize(frames, ref_u8, dev, short_side):
    from whmr_amd.demo import full_image_input_pillow
    x, u8 = full_image_input_pillow(torch.from_numpy(frames).to(dev), short_side=short_side, want_u8=True)
    assert u8.shape == ref_u8.shape and x.shape == (ref_u8.shape[0], 3) + ref_u8.shape[1:3] and x.dtype == torch.float32
    d = np.abs(u8.cpu().numpy().astype(int) - ref_u8.astype(int))
    print('max grey-level difference %d, %d values differ' % (d.max(), (d > 0).sum()))
    assert np.array_equal(u8.cpu().numpy(), ref_u8)
    want = _normalised_by_torch(u8, dev)
    print('fp32 output: %d values differ from torch on the device' % (x != want).sum().item())
    assert torch.equal(x, want)
    cpu = np.stack([FR.normalise(f) for f in ref_u8])                              # the same expression in numpy on the host: true divisions
    assert np.array_equal(x.cpu().numpy(), cpu)
    x2, u82 = full_image_input_pillow(torch.from_numpy(frames).to(dev), short_side=short_side, want_u8=True)      # cached tap tables
    assert torch.equal(x2, x) and torch.equal(u82, u8)
    assert torch.equal(full_image_input_pillow(torch.from_numpy(frames).to(dev), short_side=short_side), x)      # without the uint8 output


@pytest.mark.parametrize('case', CASES)
def test_resize_equals_pillow(dev, gold, case):
    from whmr_amd import _lib as L
    img, ref = gold['in_' + case], gold['out_' + case]
    n_tables = len(L._resize_coefs)
    _check_resize(img[None], ref[None], dev, int(gold['short_side']))
    assert len(L._resize_coefs) == n_tables + 1                                    # built once for this size, reused by the later calls


def test_resize_equals_pillow_stack(dev, gold):
    _check_resize(gold['in_stack'], gold['out_stack'], dev, int(gold['short_side']))


@pytest.mark.parametrize('size', ONE_AXIS)
def test_resize_free_sizes_equal_the_restatement(dev, size):
    """sizes the short-side rule never asks for, through the C entry: exactly one axis copied, a support of 8 taps, up in one axis and down in the
    other; two frames, the second row-group of four pixels incomplete"""
    from whmr_amd import _lib as L
    from whmr_amd.datasets.img_utils import MEAN, STD
    (H, W), (h, w) = size
    frames = np.random.default_rng(H * W).integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
    ref = np.stack([FR.resize_bilinear_u8(f, h, w) for f in frames])
    mid = torch.empty(2 * H * L.resize_mid_pitch(w), dtype=torch.uint8, device=dev)
    out, u8 = torch.empty(2, 3, h, w, device=dev), torch.empty(2, h, w, 3, dtype=torch.uint8, device=dev)
    L.resize_normalize_frames(torch.from_numpy(frames).to(dev), h, w, L.resize_coeffs(H, W, h, w, dev), mid, out, u8, MEAN, STD)
    assert np.array_equal(u8.cpu().numpy(), ref)
    assert np.array_equal(out.cpu().numpy(), np.stack([FR.normalise(f) for f in ref]))


def test_crops_of_a_clip_equal_the_per_frame_crops(dev):
    from whmr_amd.datasets.img_utils import crop_persons, crop_persons_frames
    rng = np.random.default_rng(7)
    f0 = torch.from_numpy(rng.integers(0, 256, size=(97, 131, 3), dtype=np.uint8)).to(dev)
    f1 = torch.from_numpy(rng.integers(0, 256, size=(240, 320, 3), dtype=np.uint8)).to(dev)
    wide = torch.from_numpy(rng.integers(0, 256, size=(64, 80, 3), dtype=np.uint8)).to(dev)
    f2 = wide[:, 16:64]                                                             # 64 x 48, rows 240 bytes apart
    assert not f2.is_contiguous() and f2.stride() == (240, 3, 1)
    frames = [f0, f1, f2]
    dets = [[(60.0, 50.0, 80.0, 80.0), (120.5, 10.25, 90.0, 90.0)],               # the second box leaves its frame at the top and on the right
            [],
            [(24.0, 32.0, 40.0, 40.0), (20.0, 30.0, 300.0, 300.0), (40.3, 60.7, 33.3, 33.3)]]      # the middle one is larger than its frame
    for x_slice in (None, (32, 224)):
        out, raw, index = crop_persons_frames(frames, dets, x_slice=x_slice, want_raw=True)
        assert index.tolist() == [0, 0, 2, 2, 2] and index.dtype == torch.int64 and index.is_cuda
        want = [crop_persons(f, d, x_slice=x_slice, want_raw=True) for f, d in zip(frames, dets) if d]
        assert torch.equal(out, torch.cat([w[0] for w in want])) and torch.equal(raw, torch.cat([w[1] for w in want]))
        assert raw.float().std() > 10                                              # pictures, not zeros
        only, index2 = crop_persons_frames(frames, dets, x_slice=x_slice)
        assert torch.equal(only, out) and torch.equal(index2, index)
    stack = torch.from_numpy(rng.integers(0, 256, size=(2, 50, 70, 3), dtype=np.uint8)).to(dev)      # one [F, H, W, 3] tensor; numpy frames
    a, _ = crop_persons_frames(stack, [[(30.0, 20.0, 40.0, 40.0)], [(10.0, 10.0, 25.0, 25.0)]])
    b, _ = crop_persons_frames([f.cpu().numpy() for f in stack], [[(30.0, 20.0, 40.0, 40.0)], [(10.0, 10.0, 25.0, 25.0)]])
    assert torch.equal(a, b) and torch.equal(a[1:], crop_persons(stack[1], [(10.0, 10.0, 25.0, 25.0)]))


def _inputs(dev, B, seed=0):
    from oracle import synth
    inp = synth.make_inputs(B, seed)
    return {k: inp[k].to(dev) for k in ('x', 'center', 'scale', 'bbox_height', 'orig_shape', 'bbox_info')}


def _call(model, d, rows, full_x, frame_index=None):
    return model(d['x'][rows], None, d['center'][rows], d['scale'][rows], d['bbox_height'][rows], d['orig_shape'][rows], d['bbox_info'][rows],
                 is_train=False, full_x=full_x, frame_index=frame_index)


def test_frame_index_gives_each_person_the_camera_of_their_frame(dev, model):
    d = _inputs(dev, 3)
    full = torch.randn(2, 3, 160, 224, generator=torch.Generator().manual_seed(4)).to(dev)
    out = _call(model, d, slice(0, 3), full, torch.tensor([0, 1, 1], device=dev))
    per = [_call(model, d, slice(0, 1), full[0:1]), _call(model, d, slice(1, 3), full[1:2])]
    for k, v in out.items():
        want = torch.cat([per[0][k], per[1][k]])
        e = ew_err(v, want)
        print('%-22s ew_err %.2e' % (k, e))
        assert e <= GATE, (k, e)
    assert torch.equal(out['cam_rotmat'][1], out['cam_rotmat'][2]) and torch.equal(out['render_rotmat'][1], out['render_rotmat'][2])
    assert not torch.equal(out['cam_rotmat'][0], out['cam_rotmat'][1])             # two frames, two cameras
    with pytest.raises(ValueError):
        _call(model, d, slice(0, 3), full)                                         # batch 2 for 3 persons without frame_index
    with pytest.raises(ValueError):
        _call(model, d, slice(0, 3), full, torch.tensor([0, 1], device=dev))


def _clip(dev, seed):
    rng = np.random.default_rng(seed)
    frames = torch.from_numpy(rng.integers(0, 256, size=(3, 90, 120, 3), dtype=np.uint8)).to(dev)
    c = rng.uniform(-4, 4, size=(3, 2))
    dets = [[(50.0 + c[0, 0], 40.0 + c[0, 1], 60.0, 60.0), (90.5 + c[1, 0], 30.0 + c[1, 1], 44.0, 44.0)], [], [(60.0 + c[2, 0], 50.0 + c[2, 1], 70.0, 70.0)]]
    return frames, dets


def test_infer_clip_equals_the_per_frame_path(dev, model):
    from whmr_amd.demo import infer_clip, infer_frame, prepare_clip, prepare_frame
    frames, dets = _clip(dev, 1)
    kw, P = prepare_clip(frames, dets)
    per_kw = [prepare_frame(f, d, full_image='pillow') for f, d in zip(frames, dets) if d]
    assert P == 3 and torch.equal(kw['x'], torch.cat([k['x'] for k in per_kw]))
    assert torch.equal(kw['full_x'][0:1], per_kw[0]['full_x']) and torch.equal(kw['full_x'][2:3], per_kw[1]['full_x'])
    for k in ('center', 'scale', 'bbox_height', 'orig_shape', 'bbox_info'):
        assert torch.equal(kw[k], torch.cat([p[k] for p in per_kw])), k
    out = infer_clip(model, frames, dets)
    assert out['frame_index'].tolist() == [0, 0, 2] and out['smpl_vertices'].shape == (3, 6890, 3)
    per = [infer_frame(model, f, d, full_image='pillow') for f, d in zip(frames, dets) if d]
    for k in per[0]:
        e = ew_err(out[k], torch.cat([p[k] for p in per]))
        print('%-22s ew_err %.2e' % (k, e))
        assert e <= GATE, (k, e)
    padded = infer_clip(model, frames, dets, pad_to=4)
    assert set(padded) == set(out)
    for k in out:
        assert padded[k].shape == out[k].shape, k
        e = ew_err(padded[k], out[k])
        assert e <= GATE, (k, e)
    no_cam = infer_clip(model, list(frames) + [frames[0][:50]], dets + [[(20.0, 20.0, 30.0, 30.0)]], with_full_image=False)      # mixed sizes
    assert no_cam['frame_index'].tolist() == [0, 0, 2, 3] and torch.isfinite(no_cam['smpl_vertices']).all()


def test_clip_pipeline_replays_the_eager_result(dev, model):
    import mesh_render_reference as MR
    from whmr_amd.demo import ClipPipeline, infer_clip, render_frame
    from whmr_amd.utils.renderer_cam import MeshRenderer
    pipe = ClipPipeline(model, person_bucket=4)
    for seed in (1, 2):                                                            # the second clip: same key, other pixels and boxes
        frames, dets = _clip(dev, seed)
        eager = infer_clip(model, frames, dets, pad_to=4)
        out = pipe(frames, dets)
        assert set(out) == set(eager) and len(pipe._graphs) == 1
        for k in eager:
            assert torch.equal(out[k], eager[k]), (seed, k)
    assert pipe(frames, [[], [], []]) is None
    r = MeshRenderer(MR.uv_sphere()[1])
    with_pic = ClipPipeline(model, person_bucket=4, renderer=r)
    out, images = with_pic(frames, dets)
    assert len(images) == 3 and all(i.shape == (90, 120, 3) and i.dtype == torch.uint8 for i in images)
    assert torch.equal(images[1], frames[1])                                       # the frame without a person is returned unchanged
    rows = {k: out[k][0:2] for k in ('local_smpl_vertices', 'pred_cam_t', 'focal_length')}
    assert torch.equal(images[0], render_frame(rows, frames[0], r))
