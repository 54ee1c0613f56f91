"""Generate tests/golden/whmr_losses.npz from the REAL reference's loss methods -- build container only (needs /root/reference).

    python tests/golden/make_golden_losses.py

core/trainer.py cannot be imported here (joblib, skimage, pare, the datasets, a renderer ...), and only four small methods of ``Trainer`` are
wanted: ``keypoint_loss``, ``keypoint_3d_loss``, ``shape_loss`` and ``smpl_losses`` (core/trainer.py:203-253).  They are taken from the file's syntax
tree at generation time, compiled unmodified, and called on a ``SimpleNamespace`` that holds the three criteria of :100-105 and device = 'cpu';
``batch_rodrigues`` (which ``smpl_losses`` calls) is the reference's own utils/geometry.py, imported with the stub recipe of make_golden.py.
Inputs are float64 (tests/whmr_loss_reference.py::make_case: B = 5, 37 / 11 / 5 vertices) under four mask patterns; the fixture holds the inputs
and what the methods returned -- plain arrays of a few KB, no program text.  The restatement is checked against them before anything is written.
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

import whmr_loss_reference as WR            # noqa: E402

METHODS = ('keypoint_loss', 'keypoint_3d_loss', 'shape_loss', 'smpl_losses')
CASES = {'mixed': ([1, 0, 1, 1, 0], [0, 1, 1, 0, 1]), 'all': ([1] * 5, [1] * 5), 'none': ([0] * 5, [0] * 5), 'one': ([0, 0, 0, 1, 0], [0, 1, 0, 0, 0])}
V = (37, 11, 5)


def reference_methods():
    import make_golden as MG
    MG.install_stubs()
    sys.path.insert(0, REF)
    import utils.geometry as RG
    tree = ast.parse(open(os.path.join(REF, 'core', 'trainer.py')).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'Trainer')
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(f.name for f in fns) == sorted(METHODS)
    ns = {'torch': torch, 'batch_rodrigues': RG.batch_rodrigues}
    exec(compile(ast.Module(body=fns, type_ignores=[]), 'core/trainer.py', 'exec'), ns)
    # core/trainer.py:100-105
    self = types.SimpleNamespace(criterion_shape=nn.L1Loss(), criterion_keypoints=nn.MSELoss(reduction='none'), criterion_regr=nn.MSELoss(), device='cpu')
    return {m: (lambda *a, _f=ns[m]: _f(self, *a)) for m in METHODS}


def main():
    ref = reference_methods()
    out = {}
    for ci, (name, (hs, h3)) in enumerate(CASES.items()):
        preds, tgt = WR.make_case(5, V, 100 + ci, hs, h3, all_on=True)
        p = preds[2]
        hs_b, h3_b = tgt['has_smpl'].bool(), tgt['has_pose_3d'].bool()             # core/trainer.py:389-390
        got = {}
        got['regr_pose'], got['regr_betas'] = ref['smpl_losses'](p['rotmat'], p['shape'], tgt['gt_pose'], tgt['gt_betas'], hs_b)
        got['keypoints_3d'] = ref['keypoint_3d_loss'](p['kp_3d'], tgt['pose_3d'], h3_b)
        for k in ('verts', 'sub_verts', 'temp_verts'):
            got['shape_' + k] = ref['shape_loss'](p[k], tgt['gt_' + k], hs_b)
        got['keypoints'] = ref['keypoint_loss'](p['kp_2d'], tgt['gt_kp_2d'], 0.5, 1.0)
        got['keypoints_world'] = ref['keypoint_loss'](p['kp_2d_w'], tgt['gt_kp_2d_w'], 0.5, 1.0)
        got = {k: v.double().reshape(-1)[0] if v.numel() == 1 else v.double() for k, v in got.items()}      # the empty case returns FloatTensor(1)
        mine = dict(zip(('regr_pose', 'regr_betas'), WR.smpl_losses(p['rotmat'], p['shape'], tgt['gt_pose'], tgt['gt_betas'], tgt['has_smpl'])))
        mine['keypoints_3d'] = WR.keypoint_3d_loss(p['kp_3d'], tgt['pose_3d'], tgt['has_pose_3d'])
        for k in ('verts', 'sub_verts', 'temp_verts'):
            mine['shape_' + k] = WR.shape_loss(p[k], tgt['gt_' + k], tgt['has_smpl'])
        mine['keypoints'] = WR.keypoint_loss(p['kp_2d'], tgt['gt_kp_2d'], 0.5, 1.0)
        mine['keypoints_world'] = WR.keypoint_loss(p['kp_2d_w'], tgt['gt_kp_2d_w'], 0.5, 1.0)
        for k, v in got.items():
            err = (mine[k] - v).abs().max().item() / max(v.abs().max().item(), 1e-300)
            print('  %-6s %-18s reference %-12.6g restatement max-rel %.1e' % (name, k, v.reshape(-1)[0].item(), err))
            assert err < 1e-12, (name, k, err)
            out['%s_out_%s' % (name, k)] = v.numpy()
        for k, v in tgt.items():
            out['%s_in_%s' % (name, k)] = v.numpy()
        for k, v in p.items():
            out['%s_in_pred_%s' % (name, k)] = v.numpy()
    path = os.path.join(HERE, 'whmr_losses.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
