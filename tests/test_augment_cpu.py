"""Training-batch maker, host side: the numpy restatement (tests/augment_reference.py) against the fixture recorded from the imported reference
(tests/golden/augment.npz, tests/golden/make_golden_augment.py), the package's random draws and host geometry."""
import os

import numpy as np
import pytest
import torch

import augment_reference as AR
from conftest import GOLDEN

EXACT = ('keypoints', 'smpl_2dkps', 'keypoints_world', 'betas', 'has_smpl', 'has_pose_3d', 'scale', 'center', 'orig_shape', 'is_flipped', 'rot_angle',
         'gender', 'sample_index', 'bbox_height', 'bbox_width', 'focal', 'bbox_info')
CLOSE = ('pose', 'pose_3d')                   # through rot_aa / the in-plane rotation: <= 1e-6 absolute against the stored float32


@pytest.fixture(scope='module')
def gold():
    g = dict(np.load(os.path.join(GOLDEN, 'augment.npz')))
    g['images'] = [g['image%d' % i] for i in range(3)]
    g['lab'] = {k[4:]: v for k, v in g.items() if k.startswith('ann_') and k != 'ann_img_of'}
    return g


def sets_of(g):
    for n in range(len(g['set_sample'])):
        yield n, int(g['set_sample'][n]), int(g['set_flip'][n]), float(g['set_rot'][n]), float(g['set_sc'][n]), g['set_pn'][n], bool(g['set_is_smpl'][n])


def test_restated_labels_equal_the_reference(gold):
    assert len(gold['set_sample']) >= 12 and set(np.round(gold['set_rot'], 1)) == {0.0, 17.3, -17.3, 60.0}
    worst = {k: 0.0 for k in CLOSE}
    for n, idx, flip, rot, sc, pn, is_smpl in sets_of(gold):
        shape = gold['images'][gold['ann_img_of'][idx]].shape[:2]
        mine = AR.make_labels(gold['lab'], idx, shape, flip, rot, sc, is_smpl)
        for k in EXACT:
            ref = gold['lab_' + k][n]
            assert np.asarray(mine[k]).dtype == ref.dtype, (k, np.asarray(mine[k]).dtype, ref.dtype)
            assert np.array_equal(np.asarray(mine[k]), ref), (n, k)
        for k in CLOSE:
            ref = gold['lab_' + k][n]
            assert mine[k].dtype == ref.dtype == np.float32
            worst[k] = max(worst[k], float(np.abs(mine[k].astype(np.float64) - ref).max()))
    print('restatement vs reference, max abs:', worst)
    assert all(v <= 1e-6 for v in worst.values()), worst


def test_flip_permutations_are_the_references(gold):
    from whmr_amd.core import constants as K
    for name, key in (('SMPL_JOINTS_FLIP_PERM', 'perm_smpl_joints'), ('J24_FLIP_PERM', 'perm_j24'), ('J49_FLIP_PERM', 'perm_j49'),
                      ('SMPL_J49_FLIP_PERM', 'perm_smpl_j49'), ('SMPL_POSE_FLIP_PERM', 'perm_smpl_pose')):
        assert np.array_equal(getattr(K, name), gold[key]) and np.array_equal(getattr(AR, name), gold[key]), name


def test_restated_image_equals_the_reference_at_rot_0(gold):
    """stages 1, 3, 4, 5 against BaseDataset.rgb_processing (Pillow 12.2's Image.resize): the uint8 patch exactly, the normalised tensor <= 1e-6"""
    seen = 0
    for n, idx, flip, rot, sc, pn, is_smpl in sets_of(gold):
        if 'img_%d' % n not in gold:
            continue
        seen += 1
        img = gold['images'][gold['ann_img_of'][idx]]
        patch = AR.rgb_patch(img, gold['lab']['center'][idx], sc * gold['lab']['scale'][idx], 0, flip, pn)
        ref = gold['img_%d' % n]                                               # [256, 192, 3] uint8 = 255 x the reference's float32 output
        assert np.array_equal(patch[:, AR.X0:AR.X1], ref), n
        rgb = np.transpose(ref.astype(np.float32) / np.float32(255.0), (2, 0, 1))
        norm_ref = (rgb - AR.MEAN[:, None, None]) / AR.STD[:, None, None]
        assert np.abs(AR.normalise(patch) - norm_ref).max() <= 1e-6
    assert seen >= 6


def test_draws_equal_the_references_under_its_seed(gold):
    from whmr_amd.datasets import draw_augm_params, draw_meta_mask
    n = len(gold['draw_flip'])
    np.random.seed(int(gold['seed']))
    flip, pn, rot, sc = draw_augm_params(n)
    assert np.array_equal(flip, gold['draw_flip']) and np.array_equal(pn, gold['draw_pn'])
    assert np.array_equal(rot, gold['draw_rot']) and np.array_equal(sc, gold['draw_sc'])
    assert 0 < flip.sum() < n and 0 < (rot != 0).sum() < n
    np.random.seed(int(gold['seed']) + 1)
    mask = draw_meta_mask(n)
    assert np.array_equal(mask, gold['mask'].reshape(n, 431)) and mask.min() == 0
    f2, p2, r2, s2 = draw_augm_params(5, is_train=False)
    assert not f2.any() and (p2 == 1).all() and not r2.any() and (s2 == 1).all() and draw_meta_mask(3, is_train=False).all()


def test_host_geometry_of_the_package_equals_the_restatement(gold):
    from whmr_amd.datasets import train_batch as TB
    for n, idx, flip, rot, sc, pn, is_smpl in sets_of(gold):
        c, s = gold['lab']['center'][idx], sc * gold['lab']['scale'][idx]
        ul0, br0, pad, ul, br = AR.crop_geometry(c, s, rot)
        ul_p, br_p, pad_p = TB.crop_geometry(c, s, rot)
        assert np.array_equal(ul_p, ul0) and np.array_equal(br_p, br0) and pad_p == pad
        assert np.array_equal(TB._get_transform(c, s, rot), AR.get_transform(c, s, rot))


def test_rotation_in_fp32_flips_few_grey_levels(gold):
    """the cap of tests/test_augment_gpu.py::test_rotated_patches (0.5 % of a patch's values may differ from the float64 restatement) against what
    rounding alone does: the restatement with the bilinear interpolation in float32 against itself in float64, on every rot != 0 set of the fixture.
    Measured: at most 0.0020 % of the values of a patch differ (by up to two grey levels) -- under a tenth of the cap (0.05 %)."""
    worst = 0.0
    for n, idx, flip, rot, sc, pn, is_smpl in sets_of(gold):
        if rot == 0:
            continue
        img = gold['images'][gold['ann_img_of'][idx]]
        c, s = gold['lab']['center'][idx], sc * gold['lab']['scale'][idx]
        a = AR.rgb_patch(img, c, s, rot, flip, pn, np.float64)[:, AR.X0:AR.X1].astype(int)
        b = AR.rgb_patch(img, c, s, rot, flip, pn, np.float32)[:, AR.X0:AR.X1].astype(int)
        share = float((a != b).mean())
        print('set %d rot %.1f: %.4f %% differ, max %d' % (n, rot, 100 * share, np.abs(a - b).max()))
        worst = max(worst, share)
        assert np.abs(a - b).max() <= 2
    assert worst <= 0.0005, worst


def test_flat_saturated_region_survives_rotation_and_resize():
    """v00 + a (v01 - v00) gives a flat region its value exactly: 255 stays 255 through the truncation"""
    img = np.full((120, 120, 3), 255, dtype=np.uint8)
    for dtype in (np.float64, np.float32):
        p = AR.rgb_patch(img, [60.0, 60.0], 0.2, 33.3, 0, [1.0, 1.0, 1.0], dtype)
        assert (p == 255).all()


def test_maker_refuses_the_cpu(gold):
    from whmr_amd.datasets import TrainBatchMaker
    with pytest.raises(RuntimeError):
        TrainBatchMaker(gold['lab'], torch.device('cpu'))
