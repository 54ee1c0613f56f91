"""Synthetic occluders of the training-batch maker on the device (stage 4a of csrc/augment.hip, ``TrainBatchMaker(..., occluders=)``) against the
integer / float32 restatement tests/occlusion_reference.py: exact equality, nothing in the definition leaves room for a tolerance."""
import random

import numpy as np
import pytest
import torch

import augment_reference as AR
import occlusion_reference as OR

pytestmark = pytest.mark.gpu

SIZES = ((80, 96), (220, 300), (150, 200), (100, 280))                       # H x W of the four source images
FLIP, ROT, SC = np.array([0, 1, 1, 0]), np.array([0.0, 0.0, 25.0, 0.0]), np.array([1.0, 0.9, 1.1, 1.0])
FIRST = (3, 1.0, 128, 128)                                                    # the 128 x 96 object as it is: 96 x 128 of the 192 x 256 kept pixels
PASTES = [
    [FIRST, (0, 1.0, 60.5, 70.5), (1, 0.5, 100, 30), (2, 0.73, 120, 100),     # 1 x 1; 5 x 7 halved (ties); overlaps the first
     (2, 1.0, 30, 60), (3, 0.5, 150, 250), (1, 1.0, 10, 10)],                 # over column 32; over row 255; left of the kept columns
    [FIRST, (3, 0.2, 200, 40), (2, 0.5, 225, 128), (0, 0.2, 100, 100), (3, 0.73, 100, 150)],       # over column 224; size 0; overlaps the first
    [FIRST, (2, 0.2, 50, 50), (1, 0.5, 128.5, 127.5), (3, 0.73, 128, 10), (2, 1.0, 128, 300)],     # over row 0; below the patch
    [FIRST, (3, 0.73, 40, 200), (2, 0.5, 33, 3), (1, 0.2, 128, 128), (3, 1.0, 200, 230), (2, 0.73, 90, 90), (3, 0.5, 128, 128)],   # seven, all kept
]


@pytest.fixture(scope='module')
def case(dev):
    """inputs, the device's bank-less base patches (pn = 1), the bank-less call with pn, the occluded call, and the expected occluded patches"""
    from whmr_amd.datasets import TrainBatchMaker
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
    lab = {'center': np.array([[48.0, 40.0], [150.0, 110.0], [101.3, 77.7], [140.0, 50.0]]), 'scale': np.array([0.5, 0.9, 0.6, 0.45]),
           'pose': rng.normal(0, 0.3, (4, 72)), 'shape': rng.normal(0, 1, (4, 10)), 'S': rng.normal(0, 0.4, (4, 24, 4)),
           'part': np.concatenate([rng.uniform(0, 200, (4, 24, 2)), np.ones((4, 24, 1))], -1)}          # sample 0: a 100 px box on an 80 x 96 image
    occluders = []
    for h, w in ((1, 1), (5, 7), (40, 33), (128, 96)):
        o = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
        kind = rng.random((h, w))
        o[..., 3] = np.where(kind < 0.1, 0, np.where(kind < 0.4, 255, rng.integers(64, 192, (h, w))))
        occluders.append(o)
    for o in occluders[1:]:
        o[0, 0, 3], o[0, -1, 3] = 0, 255
    occluders[0][0, 0, 3] = 180
    assert all(set(np.unique(o[..., 3])) >= {0, 255} and ((o[..., 3] > 0) & (o[..., 3] < 255)).any() for o in occluders[1:])
    pn = rng.uniform(0.6, 1.4, (4, 3))
    mask = rng.integers(0, 2, (4, 431)).astype(np.uint8)
    on_dev = [torch.from_numpy(im).to(dev) for im in images]
    idx = [0, 1, 2, 3]
    occ = [np.array(p, dtype=np.float64) for p in PASTES]
    plain, maker = TrainBatchMaker(lab, dev), TrainBatchMaker(lab, dev, occluders=occluders)
    host = lambda out: {k: v.cpu().numpy() for k, v in out.items()}
    base = host(plain(on_dev, idx, params=(FLIP, np.ones((4, 3)), ROT, SC), meta_mask=mask, want_raw=True))['img_u8']
    bare = host(plain(on_dev, idx, params=(FLIP, pn, ROT, SC), meta_mask=mask, want_raw=True))
    got = host(maker(on_dev, idx, params=(FLIP, pn, ROT, SC), meta_mask=mask, want_raw=True, occlusions=occ))
    occluded = [OR.occlude_patch(np.pad(base[b], ((0, 0), (32, 32), (0, 0))), occluders, occ[b]) for b in range(4)]
    return dict(images=images, on_dev=on_dev, lab=lab, occluders=occluders, pn=pn, mask=mask, occ=occ, idx=idx, plain=plain, maker=maker, base=base,
                bare=bare, got=got, occluded=occluded, host=host)


def _after_pn(patch, pn):
    return np.minimum(255.0, np.maximum(0.0, patch.astype(np.float64) * pn)).astype(np.uint8)


def test_occluded_batch_equals_the_restatement(case):
    """base patch = the device's own bank-less patch with pn = 1 (the path tests/test_augment_gpu.py pins); expected = occlude_patch, then pn,
    then the normalisation, in numpy; img_u8 and img equal it element for element"""
    for b in range(4):
        ref = case['occluded'][b][:, OR.X0:OR.X1]
        changed = (ref != case['base'][b]).any(-1).mean()
        print('sample %d: %.1f %% of the kept pixels occluded' % (b, 100 * changed))
        assert changed >= 0.20, (b, changed)                        # the first paste alone covers 25 %: no vacuous pass
    for b in range(4):
        want = _after_pn(case['occluded'][b], case['pn'][b])
        d = np.abs(case['got']['img_u8'][b].astype(int) - want[:, OR.X0:OR.X1].astype(int))
        print('sample %d: max grey-level difference %d, %d values differ' % (b, d.max(), (d > 0).sum()))
        assert np.array_equal(case['got']['img_u8'][b], want[:, OR.X0:OR.X1]), b
        assert np.array_equal(case['got']['img'][b], AR.normalise(want)), b


def test_rot0_sample_end_to_end_from_the_restated_pieces(case):
    """sample 1 (flipped, rot = 0) without the device's base patch: box, Pillow resize, flip, occluders, pn from the numpy restatements alone"""
    b = 1
    center, scale = case['lab']['center'][b], SC[b] * case['lab']['scale'][b]
    ul0, br0, _, _, _ = AR.crop_geometry(center, scale, 0.0)
    patch = AR.resize_bicubic_u8(AR.box_pixels(case['images'][b], ul0, br0))[:, ::-1]
    want = _after_pn(OR.occlude_patch(patch, case['occluders'], case['occ'][b]), case['pn'][b])
    assert np.array_equal(case['got']['img_u8'][b], want[:, OR.X0:OR.X1])
    assert np.array_equal(case['got']['img'][b], AR.normalise(want))


def test_no_pastes_and_labels_equal_the_bankless_call(case):
    kw = dict(params=(FLIP, case['pn'], ROT, SC), meta_mask=case['mask'], want_raw=True)
    empty = case['host'](case['maker'](case['on_dev'], case['idx'], occlusions=[np.zeros((0, 4))] * 4, **kw))
    assert set(empty) == set(case['bare']) and all(np.array_equal(empty[k], case['bare'][k]) for k in empty)
    outside = case['host'](case['maker'](case['on_dev'], case['idx'], occlusions=[np.array([(1, 1.0, 10, 10), (0, 0.2, 100, 100)])] * 4, **kw))
    assert all(np.array_equal(outside[k], case['bare'][k]) for k in outside)          # nothing survives the plan: the plain kernels run
    labels = [k for k in case['bare'] if k not in ('img', 'img_u8')]
    assert len(labels) >= 20 and all(np.array_equal(case['got'][k], case['bare'][k]) for k in labels)
    assert not np.array_equal(case['got']['img'], case['bare']['img'])
    not_train = type(case['maker'])(case['lab'], case['maker'].device, is_train=False, occluders=case['maker'].bank)
    quiet = case['host'](not_train(case['on_dev'], case['idx'], **kw))                # no draws outside training
    assert np.array_equal(quiet['img'], case['bare']['img'])


def test_same_occlusions_same_bits_and_bad_calls_raise(case):
    kw = dict(params=(FLIP, case['pn'], ROT, SC), meta_mask=case['mask'], want_raw=True)
    again = case['host'](case['maker'](case['on_dev'], case['idx'], occlusions=case['occ'], **kw))
    assert set(again) == set(case['got']) and all(np.array_equal(again[k], case['got'][k]) for k in again)
    with pytest.raises(ValueError):
        case['plain'](case['on_dev'], case['idx'], occlusions=case['occ'], **kw)
    with pytest.raises(ValueError):
        case['maker'](case['on_dev'], case['idx'], occlusions=[np.array([(4, 0.5, 100, 100)])] * 4, **kw)


def test_entry_point_rejects_inconsistent_tables(case, dev):
    """whmr_augment_crop_occluded refuses, before any launch: pastes without a bank, negative counts"""
    from whmr_amd import _lib as L
    lib, bank = L.lib(), case['maker'].bank
    z = torch.zeros(64, dtype=torch.int32, device=dev)
    m3 = (L.C.c_float * 3)(0, 0, 0)
    call = lambda bank_ptr, n_obj, n_pastes: lib.whmr_augment_crop_occluded(z.data_ptr(), 1, 8, 8, 0, None, z.data_ptr(), z.data_ptr(), z.data_ptr(), None,
                                                                            m3, m3, bank_ptr, bank.bank.numel(), bank.table.data_ptr(), n_obj,
                                                                            z.data_ptr(), z.data_ptr(), n_pastes, None)
    assert call(None, 4, 1) != 0 and call(bank.bank.data_ptr(), 4, -1) != 0 and call(bank.bank.data_ptr(), -1, 1) != 0
    assert call(bank.bank.data_ptr(), 0, 1) != 0 and call(bank.bank.data_ptr() + 1, 4, 1) != 0


def test_drawn_occlusions_change_the_image_and_feed_the_training_forward(case, dev, assets, state_dict):
    from oracle import train as OT
    from whmr_amd.models import whmr_net
    np.random.seed(3)
    random.seed(3)
    batch = case['maker'](case['on_dev'], case['idx'])
    np.random.seed(3)
    bare = case['plain'](case['on_dev'], case['idx'])                      # the same params (drawn first); no occluders
    assert batch['img'].shape == (4, 3, 256, 192) and torch.isfinite(batch['img']).all()
    assert (batch['img'] != bare['img']).any()
    for k in ('is_flipped', 'rot_angle', 'scale', 'keypoints'):
        assert torch.equal(batch[k], bare[k]), k
    m = whmr_net(None, assets=assets, numerics='fp32')
    m.load_state_dict(state_dict, strict=False)
    m = m.to(dev).train()
    out_list, _ = m(batch['img'], batch['meta_mask'], batch['center'], batch['scale'], batch['bbox_height'], batch['orig_shape'], batch['bbox_info'],
                    is_train=True)
    loss = OT.cotangent_loss(out_list['smpl_out'], dev=dev)
    loss.backward()
    assert torch.isfinite(loss)
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
