"""The training objective (whmr_amd.train.objective, csrc/whmr_loss.hip): what can be checked without a device -- the float64 restatement against the
reference's own loss methods (tests/golden/whmr_losses.npz) and the refusal of host tensors."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import whmr_loss_reference as WR

CASES = ('mixed', 'all', 'none', 'one')


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference_methods(case):
    """tests/whmr_loss_reference.py (mask multiplication, no gather) == keypoint_loss / keypoint_3d_loss / shape_loss / smpl_losses of the
    reference's Trainer on the fixture's inputs, in float64, to 1e-12 relative -- under every mask pattern, the empty one included"""
    path = os.path.join(GOLDEN, 'whmr_losses.npz')
    assert os.path.getsize(path) < 300 * 1024
    g = np.load(path)
    t = lambda k: torch.from_numpy(g['%s_in_%s' % (case, k)])
    out = lambda k: torch.from_numpy(np.asarray(g['%s_out_%s' % (case, k)]))
    assert t('gt_pose').dtype == torch.float64 and t('gt_pose').shape == (5, 72) and t('gt_verts').shape == (5, 37, 3)
    n_smpl, n_3d = int(t('has_smpl').sum()), int(t('has_pose_3d').sum())
    assert (n_smpl, n_3d) == {'mixed': (3, 3), 'all': (5, 5), 'none': (0, 0), 'one': (1, 1)}[case]
    lp, lb = WR.smpl_losses(t('pred_rotmat'), t('pred_shape'), t('gt_pose'), t('gt_betas'), t('has_smpl'))
    assert _rel(lp, out('regr_pose')) < 1e-12 and _rel(lb, out('regr_betas')) < 1e-12
    assert _rel(WR.keypoint_3d_loss(t('pred_kp_3d'), t('pose_3d'), t('has_pose_3d')), out('keypoints_3d')) < 1e-12
    for k in ('verts', 'sub_verts', 'temp_verts'):
        assert _rel(WR.shape_loss(t('pred_' + k), t('gt_' + k), t('has_smpl')), out('shape_' + k)) < 1e-12
    assert _rel(WR.keypoint_loss(t('pred_kp_2d'), t('gt_kp_2d'), 0.5, 1.0), out('keypoints')) < 1e-12
    assert _rel(WR.keypoint_loss(t('pred_kp_2d_w'), t('gt_kp_2d_w'), 0.5, 1.0), out('keypoints_world')) < 1e-12
    if case == 'none':                                   # the reference's `else` branches: exact zeros
        assert lp.item() == 0.0 and lb.item() == 0.0 and out('regr_pose').item() == 0.0 and out('shape_verts').item() == 0.0


def test_restatement_key_sets_and_finite_gradients_without_a_valid_sample():
    """15 keys in the default configuration, 24 with every optional term (core/trainer.py:538-587); with empty masks the masked terms are 0.0 and
    autograd through the restatement gives finite, all-zero gradients (the clamp, not a division by zero)"""
    for all_on, n in ((False, 15), (True, 24)):
        preds, tgt = WR.make_case(3, (37, 11, 5), 1, [0, 0, 0], [0, 0, 0], all_on=all_on)
        preds, tgt = WR.to(preds, tgt, requires_grad=True)
        d = WR.loss_dict(preds, tgt, WR.ALL_ON_W if all_on else WR.DEFAULT_W)
        assert len(d) == n and list(d)[:2] == ['loss_regr_pose_1', 'loss_regr_betas_1'] and list(d)[-1] == 'loss_cam_3'
        torch.stack(list(d.values())).sum().backward()
        for k in ('loss_regr_pose_2', 'loss_regr_betas_1', 'loss_keypoints_3d_3', 'loss_shape_3', 'loss_shape_sub_3', 'loss_shape_temp_3'):
            assert d[k].item() == 0.0, k
        for k in ('rotmat', 'shape', 'kp_3d', 'verts'):
            assert preds[2][k].grad is not None and not preds[2][k].grad.any(), k
        assert preds[0]['cam'].grad[:, 0].abs().min() > 0 and not preds[0]['cam'].grad[:, 1:].any()


def test_objective_imports_and_refuses_host_tensors():
    """the no-CPU-fallback rule (test_host_cpu.py::test_no_cpu_fallback): the public functions raise the package's device-only error"""
    from whmr_amd import _lib
    from whmr_amd.train import WHMRLossFn, build_targets, compute_losses, total_loss
    from whmr_amd.train import objective as O
    assert len(O.TERM_KEYS) == _lib.LOSS_TERMS == len(_lib.LOSS_FIELDS) and sorted(O.DICT_ORDER) == list(range(10))
    assert _lib.LOSS_FIELDS == WR.FIELDS and _lib.LOSS_TARGETS == WR.TARGETS
    preds, tgt = WR.make_case(2, (37, 11, 5), 0, [1, 0], [1, 1], dtype=torch.float32)
    smpl_out = [None] + [dict(p, theta=torch.cat([p['cam'], p['shape'], torch.zeros(2, 72)], 1)) for p in preds]
    batch = {'pose': tgt['gt_pose'], 'betas': tgt['gt_betas'], 'pose_3d': tgt['pose_3d'], 'has_smpl': tgt['has_smpl'], 'has_pose_3d': tgt['has_pose_3d'],
             'opt_vertices': tgt['gt_verts'], 'opt_sub_vertices': tgt['gt_sub_verts'], 'opt_temp_vertices': tgt['gt_temp_verts']}
    with pytest.raises(RuntimeError, match='HIP device only'):
        compute_losses({'smpl_out': smpl_out, 'dp_out': []}, batch)
    with pytest.raises(RuntimeError, match='HIP device only'):
        WHMRLossFn.apply({}, {}, *([torch.zeros(2, 24, 3, 3)] + [None] * 29))
    with pytest.raises(RuntimeError, match='HIP device only'):
        build_targets(None, dict(batch, keypoints=torch.zeros(2, 49, 3)))
    with pytest.raises(RuntimeError):
        _lib.train_losses(preds, tgt, WR.DEFAULT_W)
    d = {'a': torch.tensor(1.5), 'b': torch.tensor(2.0)}                                  # a plain dictionary: the reference's stack-and-sum (:609)
    assert total_loss(d).item() == 3.5


def test_whmr_loss_source_is_built_without_packed_fp32():
    from whmr_amd import build
    assert 'whmr_loss.hip' in build.NO_PACKED_FP32 or os.environ.get('WHMR_BUILD_PACKED_FP32') == '1'
    assert os.path.exists(os.path.join(ROOT, 'w-hmr_amd', 'csrc', 'whmr_loss.hip'))
