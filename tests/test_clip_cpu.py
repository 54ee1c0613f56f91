"""Clip inference, the parts that need no GPU: the numpy restatement of Pillow's bilinear resize (tests/frames_reference.py) against the fixture
recorded from Pillow (tests/golden/frames.npz) and against Pillow itself where it is installed; the host-side layout of a clip (frame_index order,
padding, target size) and the ValueError paths, all of which are decided before any device call."""
import os

import numpy as np
import pytest
import torch

import frames_reference as FR
from conftest import GOLDEN
from whmr_amd import _lib as L
from whmr_amd.datasets.img_utils import frame_index_of
from whmr_amd.demo import clip_plan, padded_count, resize_target
from whmr_amd.models.whmr import check_full_x_batch

CASES = ('landscape_down', 'non_integer_ratio', 'portrait_down', 'portrait_up', 'short_side_unchanged', 'extreme_ratio')
ONE_AXIS = [((60, 83), (60, 50)), ((60, 83), (45, 83)), ((61, 480), (60, 60)), ((33, 21), (70, 8))]     # one axis copied (x2), support 8, up + down


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(GOLDEN, 'frames.npz')))


@pytest.mark.parametrize('case', CASES)
def test_restatement_equals_the_pillow_fixture(gold, case):
    img, ref = gold['in_' + case], gold['out_' + case]
    assert ref.shape[:2] == FR.resize_target(img.shape[0], img.shape[1], int(gold['short_side']))
    assert np.array_equal(FR.resize_bilinear_u8(img, *ref.shape[:2]), ref)


def test_restatement_equals_the_pillow_fixture_stack(gold):
    for img, ref in zip(gold['in_stack'], gold['out_stack']):
        assert np.array_equal(FR.resize_bilinear_u8(img, *ref.shape[:2]), ref)


def test_restatement_equals_pillow_on_fresh_sizes():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(2)
    sizes = [((int(rng.integers(8, 90)), int(rng.integers(8, 90))), (int(rng.integers(4, 70)), int(rng.integers(4, 70)))) for _ in range(12)]
    for (H, W), (h, w) in sizes + ONE_AXIS:
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img).resize((w, h), Image.BILINEAR))
        assert np.array_equal(FR.resize_bilinear_u8(img, h, w), ref), ((H, W), (h, w))


def test_target_size_rule():
    assert resize_target(720, 1280) == (600, 1066) and resize_target(1280, 720) == (1066, 600) and resize_target(360, 640) == (600, 1066)
    assert resize_target(500, 500, 60) == (60, 60) and resize_target(61, 480, 60) == (60, 472) and resize_target(40, 30, 60) == (80, 60)
    for H, W in ((75, 100), (131, 97), (60, 83)):
        assert resize_target(H, W, 60) == FR.resize_target(H, W, 60)
    assert L.resize_ksize(480, 60) == 17 and L.resize_ksize(30, 60) == 3 and L.resize_ksize(131, 81) == 5
    assert L.resize_mid_pitch(1066) == 3216 and L.resize_mid_pitch(5) == 32 and L.resize_mid_pitch(4) == 16


def test_frame_index_order_with_empty_frames():
    d = (1.0, 2.0, 3.0, 4.0)
    assert frame_index_of([[], [d, d], [], [d], []]).tolist() == [1, 1, 3]
    assert frame_index_of([[d], [], [d, d, d]]).tolist() == [0, 2, 2, 2]
    assert frame_index_of([[], []]).tolist() == [] and frame_index_of([[], []]).dtype == np.int64
    frames = [np.zeros((8, 9, 3), np.uint8)] * 4
    dets = [[], [(1, 1, 2, 2), (3, 3, 2, 2)], [], [(5, 5, 2, 2)]]
    P, Pp, shapes, flat, index = clip_plan(frames, dets)
    assert (P, Pp) == (3, 3) and index.tolist() == [1, 1, 3] and index.dtype == np.int64 and shapes == [(8, 9)] * 4
    assert flat == [(1.0, 1.0, 2.0, 2.0), (3.0, 3.0, 2.0, 2.0), (5.0, 5.0, 2.0, 2.0)]
    assert clip_plan(frames, [[], [], [], []]) is None
    assert clip_plan(np.zeros((2, 8, 9, 3), np.uint8), [[(1, 1, 2, 2)], []])[2] == [(8, 9)] * 2          # one [F, H, W, 3] block


def test_pad_to_arithmetic_and_rows():
    assert [padded_count(p, 4) for p in (1, 3, 4, 5, 8, 9)] == [4, 4, 4, 8, 8, 12]
    assert padded_count(7) == 7 and padded_count(7, 1) == 7
    with pytest.raises(ValueError):
        padded_count(3, 0)
    frames = [np.zeros((8, 9, 3), np.uint8)] * 3
    dets = [[(1, 1, 2, 2), (3, 3, 2, 2)], [(5, 5, 2, 2)], []]
    P, Pp, _, flat, index = clip_plan(frames, dets, pad_to=4)
    assert (P, Pp) == (3, 4) and index.tolist() == [0, 0, 1, 1] and flat[3] == flat[2] == (5.0, 5.0, 2.0, 2.0)
    assert np.all(np.diff(index) >= 0)                                              # padded rows keep the frame order the crop table relies on
    out = {'a': torch.arange(Pp * 2).view(Pp, 2)}
    from whmr_amd.demo import _clip_result
    res = _clip_result(out, {'frame_index': torch.from_numpy(index)}, P)
    assert res['a'].shape == (3, 2) and res['frame_index'].tolist() == [0, 0, 1]


def test_value_errors_come_before_any_device_call():
    frames = [np.zeros((8, 9, 3), np.uint8), np.zeros((9, 8, 3), np.uint8)]
    with pytest.raises(ValueError, match='one size'):
        clip_plan(frames, [[(1, 1, 2, 2)], []])
    from whmr_amd.demo import infer_clip
    with pytest.raises(ValueError, match='one size'):
        infer_clip(None, frames, [[(1, 1, 2, 2)], []])
    assert clip_plan(frames, [[(1, 1, 2, 2)], []], with_full_image=False)[0] == 1  # mixed sizes are fine without the camera input
    with pytest.raises(ValueError):
        clip_plan(frames, [[(1, 1, 2, 2)]])
    assert infer_clip(None, frames[:1] * 2, [[], []]) is None                      # no detection: nothing is uploaded, no model call
    fx = lambda n: torch.zeros(n, 3, 4, 4)
    assert check_full_x_batch(None, 3) == 'none' and check_full_x_batch(fx(1), 3) == 'broadcast' and check_full_x_batch(fx(3), 3) == 'per_person'
    assert check_full_x_batch(fx(2), 3, torch.tensor([0, 1, 1])) == 'frames' and check_full_x_batch(fx(5), 3, torch.tensor([0, 4, 4])) == 'frames'
    with pytest.raises(ValueError, match='batch 2'):
        check_full_x_batch(fx(2), 3)
    with pytest.raises(ValueError):
        check_full_x_batch(fx(2), 3, torch.tensor([0, 1]))                         # one frame index per person
    with pytest.raises(ValueError):
        check_full_x_batch(fx(2), 3, torch.tensor([0, 1, 1], dtype=torch.int32))
