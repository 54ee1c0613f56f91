"""Training-batch maker on the device (csrc/augment.hip, whmr_amd.datasets.TrainBatchMaker) against the fixture recorded from the imported
reference (tests/golden/augment.npz), its numpy restatement (tests/augment_reference.py) and an image / label consistency check that needs neither."""
import os

import numpy as np
import pytest
import torch

import augment_reference as AR
from conftest import GOLDEN
from test_augment_cpu import CLOSE, EXACT, sets_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    g = dict(np.load(os.path.join(GOLDEN, 'augment.npz')))
    g['images'] = [g['image%d' % i] for i in range(3)]
    g['lab'] = {k[4:]: v for k, v in g.items() if k.startswith('ann_') and k != 'ann_img_of'}
    return g


def _run(dev, gold, chosen, **kw):
    """one call of the maker with the parameter sets ``chosen`` of the fixture as a batch (they share kp_is_smpl)"""
    from whmr_amd.datasets import TrainBatchMaker
    maker = TrainBatchMaker(gold['lab'], dev)
    on_dev = [torch.from_numpy(im).to(dev) for im in gold['images']]
    idx = [s[1] for s in chosen]
    params = (np.array([s[2] for s in chosen]), np.stack([s[5] for s in chosen]), np.array([s[3] for s in chosen]), np.array([s[4] for s in chosen]))
    out = maker([on_dev[gold['ann_img_of'][i]] for i in idx], idx, params=params, kp_is_smpl=chosen[0][6], want_raw=True, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_labels(out, gold, chosen):
    for b, s in enumerate(chosen):
        for k in EXACT:
            ref = gold['lab_' + k][s[0]]
            assert out[k][b].dtype == ref.dtype, (k, out[k].dtype, ref.dtype)
            assert np.array_equal(out[k][b], ref), (s[0], k, out[k][b], ref)
        for k in CLOSE:
            assert np.abs(out[k][b].astype(np.float64) - gold['lab_' + k][s[0]]).max() <= 1e-6, (s[0], k)


def test_rot0_batch_equals_the_reference(dev, gold):
    """every rot = 0 set of the fixture in ONE call (three source sizes, a box that leaves its image on two sides, up- and down-sampling boxes):
    the uint8 patch exactly, img <= 1e-6, labels as in the CPU test"""
    chosen = [s for s in sets_of(gold) if s[3] == 0 and not s[6]]
    assert len(chosen) >= 6 and len({gold['ann_img_of'][s[1]] for s in chosen}) == 3
    out = _run(dev, gold, chosen)
    assert out['img'].shape == (len(chosen), 3, 256, 192) and out['img'].dtype == np.float32 and out['meta_mask'].shape == (len(chosen), 431, 1)
    for b, s in enumerate(chosen):
        ref = gold['img_%d' % s[0]]
        d = np.abs(out['img_u8'][b].astype(int) - ref.astype(int))
        print('set %d: max grey-level difference %d, %d values differ' % (s[0], d.max(), (d > 0).sum()))
        assert np.array_equal(out['img_u8'][b], ref), s[0]
        rgb = np.transpose(ref.astype(np.float32) / np.float32(255.0), (2, 0, 1))
        assert np.abs(out['img'][b] - (rgb - AR.MEAN[:, None, None]) / AR.STD[:, None, None]).max() <= 1e-6
    _check_labels(out, gold, chosen)


def test_rotated_patches(dev, gold):
    """rot != 0 against the float64 restatement: the device interpolates in fp32 and stage 2 truncates, so a value within fp32 rounding of an integer
    may land one grey level lower or higher.  Gate: no value differs by more than 2 grey levels and at most 0.5 % of a patch's values differ at all
    (tests/test_augment_cpu.py::test_rotation_in_fp32_flips_few_grey_levels measures what rounding alone does: 0.0020 %).  Labels against the
    fixture as for rot = 0, both joint conventions."""
    for is_smpl in (False, True):
        chosen = [s for s in sets_of(gold) if s[6] == is_smpl and (s[3] != 0 or is_smpl)]
        out = _run(dev, gold, chosen)
        _check_labels(out, gold, chosen)
        for b, (n, idx, flip, rot, sc, pn, _) in enumerate(chosen):
            img = gold['images'][gold['ann_img_of'][idx]]
            ref = AR.rgb_patch(img, gold['lab']['center'][idx], sc * gold['lab']['scale'][idx], rot, flip, pn)[:, AR.X0:AR.X1]
            d = np.abs(out['img_u8'][b].astype(int) - ref.astype(int))
            print('set %d rot %.1f: max grey-level difference %d, %.4f %% of the values differ' % (n, rot, d.max(), 100.0 * (d > 0).mean()))
            assert d.max() <= 2 and (d > 0).mean() <= 0.005, (n, d.max(), (d > 0).mean())
            assert np.abs(out['img'][b] - AR.normalise(np.pad(out['img_u8'][b], ((0, 0), (32, 32), (0, 0))))).max() <= 1e-6


@pytest.mark.parametrize('rot', [0.0, 25.0, -40.0])
@pytest.mark.parametrize('flip', [0, 1])
@pytest.mark.parametrize('sc', [0.8, 1.2])
def test_marks_land_on_their_keypoints(dev, rot, flip, sc):
    """image / label consistency without any restatement: bright 5 x 5 marks at known keypoints of a dark image; the centroid of each mark in
    the output patch lies within 1.5 px of the transformed keypoint (1 px from transform's integer truncation, 0.5 from the centroid of a resized
    mark).  Catches a wrong sign of rot, or a flip applied to one side only."""
    from whmr_amd.datasets import TrainBatchMaker
    H, W, c = 400, 420, np.array([210.02, 200.02])                    # box 208 / 312 px: its corner sits 0.02 px behind an integer at both scales
    pts = c - 0.02 + np.array([[-40, -50], [35, -45], [0, 10], [30, 50], [-45, 40]], dtype=np.float64)      # integer pixels, apart, inside the patch at every setting
    joints = [25 + 0, 25 + 5, 25 + 12, 25 + 13, 25 + 14]                                                 # right / left ankle (a flip pair) + 3 central
    img = np.zeros((H, W, 3), dtype=np.uint8)
    for x, y in np.rint(pts).astype(int):
        img[y - 2:y + 3, x - 2:x + 3] = 255
    part = np.zeros((1, 24, 3))
    for (x, y), j in zip(np.rint(pts), joints):
        part[0, j - 25] = [x, y, 1.0]
    maker = TrainBatchMaker({'center': c[None], 'scale': np.array([1.3]), 'part': part}, dev)
    out = maker([img], [0], params=(np.array([flip]), np.ones((1, 3)), np.array([rot]), np.array([sc])), want_raw=True)
    patch = out['img_u8'][0].cpu().numpy()[..., 0].astype(np.float64)
    kp = out['keypoints'][0].cpu().numpy()
    yy, xx = np.mgrid[0:256, 0:192]
    for j in joints:
        assert kp[j, 2] == 1.0                                        # after a flip joint j carries its mirror joint's mark: still one of the five
        px, py = (kp[j, 0] + 1) * 128 - 32, (kp[j, 1] + 1) * 128      # the label as a pixel of the 192-wide patch
        assert 8 < px < 184 and 8 < py < 248, (j, px, py)
        win = (np.abs(xx - px) < 14) & (np.abs(yy - py) < 14)
        wsum = (patch * win).sum()
        assert wsum > 255 * 8, (j, wsum)
        cx, cy = (patch * win * xx).sum() / wsum, (patch * win * yy).sum() / wsum
        # s = box / 256 = 0.81 | 1.22 source pixels per patch pixel.  The mark's centre is patch pixel t + 0.52 / s - 0.5 (t = the exact transform of
        # the keypoint), the label is trunc(t) + 1, mirrored as 256 - label while the image mirrors as 255 - pixel: label - centroid lies in
        # (-0.14, 1.07] unflipped, [-0.07, 1.14) flipped -- plus the centroid's own half pixel: 1.5.
        assert abs(px - cx) <= 1.5 and abs(py - cy) <= 1.5, (rot, flip, sc, j, (cx, cy), (px, py))


def test_same_params_same_bits_and_cpu_images_raise(dev, gold):
    chosen = [s for s in sets_of(gold) if not s[6]]
    mask = np.random.default_rng(0).integers(0, 2, (len(chosen), 431)).astype(np.uint8)
    a, b = _run(dev, gold, chosen, meta_mask=mask), _run(dev, gold, chosen, meta_mask=mask)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert np.array_equal(a['meta_mask'][..., 0], mask.astype(np.float32))
    from whmr_amd.datasets import TrainBatchMaker
    maker = TrainBatchMaker(gold['lab'], dev)
    with pytest.raises(RuntimeError):
        maker([torch.from_numpy(gold['images'][0])], [0])
    drawn = maker([gold['images'][0], gold['images'][1]], [0, 1])                                        # numpy images, drawn parameters
    assert torch.isfinite(drawn['img']).all() and drawn['meta_mask'].shape == (2, 431, 1)


def test_absent_annotations_default_as_the_reference(dev, gold):
    from whmr_amd.datasets import TrainBatchMaker
    lab = {k: gold['lab'][k] for k in ('center', 'scale', 'part')}
    out = TrainBatchMaker(lab, dev)([gold['images'][0]], [3], params=(np.array([1]), np.ones((1, 3)), np.array([17.3]), np.array([1.0])))
    ref = AR.make_labels(lab, 3, gold['images'][0].shape[:2], 1, 17.3, 1.0)
    for k in EXACT + CLOSE:
        got = out[k][0].cpu().numpy()
        assert got.dtype == np.asarray(ref[k]).dtype and np.array_equal(got, np.asarray(ref[k])), k
    assert out['gender'][0].item() == -1 and out['has_pose_3d'][0].item() == 0 and not out['pose'].any()


def test_batch_feeds_the_training_forward(dev, gold, assets, state_dict):
    """the returned dict goes through WHMR.forward(is_train=True) + backward on the synthetic weights: finite loss and gradients"""
    from oracle import train as OT
    from whmr_amd.datasets import TrainBatchMaker
    from whmr_amd.models import whmr_net
    chosen = [s for s in sets_of(gold) if not s[6]][:4]
    maker = TrainBatchMaker(gold['lab'], dev)
    idx = [s[1] for s in chosen]
    np.random.seed(3)
    batch = maker([gold['images'][gold['ann_img_of'][i]] for i in idx], idx)
    m = whmr_net(None, assets=assets, numerics='fp32')
    m.load_state_dict(state_dict, strict=False)
    m = m.to(dev).train()
    out_list, _ = m(batch['img'], batch['meta_mask'], batch['center'], batch['scale'], batch['bbox_height'], batch['orig_shape'], batch['bbox_info'],
                    is_train=True)
    loss = OT.cotangent_loss(out_list['smpl_out'], dev=dev)
    loss.backward()
    assert torch.isfinite(loss)
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
