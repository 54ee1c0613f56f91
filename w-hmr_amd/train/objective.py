"""The W-HMR training objective on the device: ``loss_dict = compute_losses(preds_dict, build_targets(model, input_batch))``.

Reference: core/trainer.py:413-464 (targets) and :466-609 (loss_dict).  The reference's loss methods gather the supervised samples with boolean
masks (``x[has_smpl]``, :221-223, :235-236, :243-246) and branch on ``len(...) > 0`` -- each a host synchronisation, so that code cannot be part
of a captured step -- and evaluate 15-24 scalar terms as a few tiny launches each.  ``WHMRLossFn`` is ONE autograd node over the three supervised
stages: csrc/whmr_loss.hip sums every term in two launches (fixed order, no atomics), counts the valid samples on the device and writes all
gradients in a third.  The dense-correspondence terms stay with ``IUVLossFn`` (train/aux_supervision.py); with cfg.MODEL.PyMAF.DEPTH_SUPV_ON they and
``loss_Depth`` (:301-317, :489-496) come from ``AuxLossFn``, one node over the 91-channel head output.
"""
import torch

from .. import _lib as L
from ..core.cfgs import cfg
from ..core.constants import FOCAL_LENGTH
from ..utils.geometry import estimate_translation
from .aux_supervision import (AuxLossFn, IUVLossFn, body_uv_losses, depth_losses, fused_aux_operand, gt_camera_from_translation, render_depth_target,
                              render_iuv_targets)
from .heads_autograd import downsample_csr
from ..utils.iuvmap import iuv_img2map

# the reference's key stems in the order of losses[stage * 10 + k] (include/whmr_hip.h), and the order core/trainer.py:538-587 fills loss_dict in
TERM_KEYS = ('loss_regr_pose', 'loss_regr_betas', 'loss_keypoints_3d', 'loss_shape', 'loss_shape_sub', 'loss_shape_temp', 'loss_cam',
             'loss_keypoints', 'loss_keypoints_world', 'loss_focal_length')
DICT_ORDER = (0, 1, 7, 8, 9, 2, 3, 4, 5, 6)
IUV_KEYS = ('loss_U', 'loss_V', 'loss_IndexUV', 'loss_segAnn')
DEPTH_KEY = 'loss_Depth'


def _f32(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


class WHMRLossFn(torch.autograd.Function):
    """losses [30] = WHMRLossFn.apply(targets, weights, *preds): ``preds`` = for each of the three stages the ten tensors of ``_lib.LOSS_FIELDS``
    (None switches a term off), ``targets`` / ``weights`` = the dictionaries of ``_lib.LOSS_TARGETS`` / ``_lib.LOSS_WEIGHTS``.  Entry
    stage * 10 + k is term ``TERM_KEYS[k]`` of ``smpl_out[stage + 1]``, weighted; a term that is off, or masked without a valid sample, is 0.0."""

    @staticmethod
    def forward(ctx, targets, weights, *preds):
        n = len(L.LOSS_FIELDS)
        assert len(preds) == L.LOSS_STAGES * n
        live = [t for t in preds if t is not None]
        if not live or not all(t.is_cuda for t in live):
            raise RuntimeError('whmr_amd runs on a HIP device only (no CPU fallback)')
        stages = []
        for s in range(L.LOSS_STAGES):
            d = {}
            for k, t in zip(L.LOSS_FIELDS, preds[s * n:(s + 1) * n]):
                if t is not None:
                    t = t.detach()
                    if t.dtype != torch.float32:
                        t = t.float()
                    if k in ('shape', 'cam'):           # a column slice is read in place
                        t = t if t.stride(1) == 1 else t.contiguous()
                    else:
                        t = t.contiguous()
                d[k] = t
            stages.append(d)
        losses, counts = L.train_losses(stages, targets, weights)
        ctx.saved = (stages, targets, dict(weights), counts)
        ctx.dtypes = [None if t is None else t.dtype for t in preds]
        return losses

    @staticmethod
    def backward(ctx, g):
        stages, targets, weights, counts = ctx.saved
        ctx.saved = None
        grads = L.train_losses_bwd(stages, targets, weights, counts, g)
        flat = [grads[s].get(k) for s in range(L.LOSS_STAGES) for k in L.LOSS_FIELDS]
        flat = [t if (t is None or t.dtype == dt) else t.to(dt) for t, dt in zip(flat, ctx.dtypes)]
        return (None, None) + tuple(flat)


class LossDict(dict):
    """``loss_dict`` of core/trainer.py:467-591.  Every value is a 0-dim view of one of ``vectors`` (the fused node's output, the IUV node's);
    entries of those vectors that have no key are exactly 0.0, so ``total_loss`` may add the vectors instead of stacking two dozen views."""
    vectors = ()


def loss_weights(options=None):
    """cfg.LOSS / options at call time -> the ``weights`` dictionary of ``WHMRLossFn`` (core/trainer.py:539-582)"""
    opt = lambda k, d: float(getattr(options, k, d) if options is not None else d)
    return {'w_pose': float(cfg.LOSS.POSE_W), 'w_shape': float(cfg.LOSS.SHAPE_W), 'w_kp3d': float(cfg.LOSS.KP_3D_W), 'w_vert': float(cfg.LOSS.VERT_W),
            'w_kp2d': float(cfg.LOSS.KP_2D_W), 'w_focal': float(cfg.LOSS.FOCAL_WEIGHTS), 'w_openpose': opt('openpose_train_weight', 0.),
            'w_gt': opt('gt_train_weight', 1.)}


def loss_targets(targets, kp_2d, focal, verts):
    """the batch / ``build_targets`` dictionary -> the ``targets`` dictionary of ``WHMRLossFn`` (fp32, contiguous; what a switched-off term needs is left out)"""
    t = {'gt_pose': targets['pose'], 'gt_betas': targets['betas'], 'pose_3d': targets['pose_3d'], 'has_smpl': targets['has_smpl'],
         'has_pose_3d': targets['has_pose_3d']}
    if verts:
        t.update(gt_verts=targets['opt_vertices'], gt_sub_verts=targets['opt_sub_vertices'], gt_temp_verts=targets['opt_temp_vertices'])
    if kp_2d:
        t.update(gt_kp_2d=targets['keypoints'], gt_kp_2d_w=targets['keypoints_world'], orig_shape=targets['orig_shape'],
                 bbox_width=targets['bbox_width'], bbox_height=targets['bbox_height'])
    if focal:
        t['gt_focal'] = targets['focal']
    for v in t.values():
        if not v.is_cuda:
            raise RuntimeError('whmr_amd runs on a HIP device only (no CPU fallback)')
    return {k: _f32(v.detach()) for k, v in t.items()}


def _iuv_terms(d, iuv_image_gt):
    """the four dense-correspondence terms of one ``dp_out`` entry, by the path ``aux_supervision_loss`` takes for it"""
    y = getattr(d, 'nhwc', None)
    if (y is not None and y.is_cuda and y.shape[-1] == 90 and tuple(iuv_image_gt.shape) == (y.shape[0], 3, y.shape[1], y.shape[2])):
        return IUVLossFn.apply(y, iuv_image_gt, float(cfg.LOSS.POINT_REGRESSION_WEIGHTS))
    lu, lv, li, la = body_uv_losses(d['predict_u'], d['predict_v'], d['predict_uv_index'], d['predict_ann_index'], iuv_img2map(iuv_image_gt))
    return torch.stack([lu, lv, li, la])


def compute_losses(preds_dict, targets, options=None):
    """core/trainer.py:466-591: ``loss_dict`` with the reference's keys (``loss_regr_pose_1`` ... ``loss_cam_3``; with cfg.MODEL.PyMAF.AUX_SUPV_ON
    and ``targets['iuv_image_gt']`` also ``loss_U-1`` ... ``loss_segAnn-1``, has_iuv = None as in ``aux_supervision_loss``; with
    cfg.MODEL.PyMAF.DEPTH_SUPV_ON, a ``dpth_out`` entry and ``targets['depth_image_gt']`` also ``loss_Depth-1``, :489-496, masked by
    ``targets['has_smpl']``).  ``targets``: the batch dictionary with the entries of ``build_targets``; ``options``: anything with
    ``openpose_train_weight`` / ``gt_train_weight`` (defaults 0. / 1.)."""
    if cfg.MODEL.PyMAF.DEPTH_SUPV_ON and not cfg.MODEL.PyMAF.AUX_SUPV_ON:
        # the reference creates its depth renderer, and renders the target, only under AUX_SUPV_ON (core/trainer.py:167-171, :442-460)
        raise ValueError('cfg.MODEL.PyMAF.DEPTH_SUPV_ON needs cfg.MODEL.PyMAF.AUX_SUPV_ON: the depth target is rendered with the IUV target')
    smpl_out = preds_dict['smpl_out']
    assert len(smpl_out) == L.LOSS_STAGES + 1, 'three supervised stages behind the mean-pose entry (core/trainer.py:508-513)'
    kp_2d, focal, verts = float(cfg.LOSS.KP_2D_W) > 0, bool(cfg.MODEL.PyMAF.FOCAL_SUPV_ON), float(cfg.LOSS.VERT_W) > 0
    flat, live = [], []
    for l in range(1, L.LOSS_STAGES + 1):
        d = smpl_out[l]
        theta = d['theta']
        on = {'rotmat': True, 'shape': True, 'kp_3d': True, 'cam': True, 'kp_2d': kp_2d, 'kp_2d_w': kp_2d, 'focal': focal,
              'verts': verts and l > 2, 'sub_verts': verts and l > 2, 'temp_verts': verts and l > 2}          # trainer.py:544, :567, :576
        # trainer.py:515-523; the package's own forward also hands out the two blocks theta was concatenated from (the same values and graph,
        # without the concatenation's backward in between)
        src = {'shape': d['pred_shape'] if 'pred_shape' in d else theta[:, 3:13], 'cam': d['pred_cam'] if 'pred_cam' in d else theta[:, :3],
               'focal': d.get('focal_length')}
        flat += [(src[k] if k in src else d[k]) if on[k] else None for k in L.LOSS_FIELDS]
        live.append([k for k in DICT_ORDER if on[L.LOSS_FIELDS[k]]])
    losses = WHMRLossFn.apply(loss_targets(targets, kp_2d, focal, verts), loss_weights(options), *flat)
    out = LossDict()
    vectors = []
    iuv = targets.get('iuv_image_gt')
    dp_out = preds_dict.get('dp_out') or []
    depth = targets.get('depth_image_gt')
    dpth_out = (preds_dict.get('dpth_out') or []) if (cfg.MODEL.PyMAF.DEPTH_SUPV_ON and depth is not None) else []
    w_point = float(cfg.LOSS.POINT_REGRESSION_WEIGHTS)
    fused = {}                                              # index into dpth_out -> its term, where AuxLossFn covered both heads' entries
    if cfg.MODEL.PyMAF.AUX_SUPV_ON and iuv is not None:                                                        # trainer.py:469-487
        for i, d in enumerate(dp_out):
            y = fused_aux_operand(d, dpth_out[i], iuv, depth) if i < len(dpth_out) else None
            if y is not None:
                v = AuxLossFn.apply(y, iuv, depth, targets.get('has_smpl'), w_point)
                fused[i] = v[4]
            else:
                v = _iuv_terms(d, iuv)
            vectors.append(v)
            for j, k in enumerate(IUV_KEYS):
                out['%s%d' % (k, i - len(dp_out))] = v[j]
    for i, d in enumerate(dpth_out):                                                                           # trainer.py:489-496
        if i in fused:
            out['%s%d' % (DEPTH_KEY, i - len(dp_out))] = fused[i]
        else:
            v = depth_losses(d, depth, targets.get('has_smpl')).reshape(1)
            vectors.append(v)
            out['%s%d' % (DEPTH_KEY, i - len(dp_out))] = v[0]
    for s, ks in enumerate(live):
        for k in ks:
            out['%s_%d' % (TERM_KEYS[k], s + 1)] = losses[s * L.LOSS_TERMS + k]
    vectors.append(losses)
    out.vectors = tuple(vectors)
    out.n_keys = len(out)
    return out


def total_loss(loss_dict):
    """core/trainer.py:609: the sum of the entries"""
    vectors = getattr(loss_dict, 'vectors', ())
    if vectors and len(loss_dict) == getattr(loss_dict, 'n_keys', -1):
        total = vectors[0].sum()
        for v in vectors[1:]:
            total = total + v.sum()
        return total
    return torch.stack(list(loss_dict.values())).sum()


@torch.no_grad()
def build_targets(model, input_batch, iuv_maker=None, img_res=224, depth_maker=None):
    """core/trainer.py:413-464 with kernels the forward already uses: SMPL of the ground-truth parameters (:415-425), the two mesh down-samplings
    (:422-423), the camera translation fitted to the 2-D keypoints (:429-436; ``img_res`` = options.img_res) and -- with ``iuv_maker`` -- the
    rendered dense-correspondence image (:442-462, valid_fit = all) and -- with ``depth_maker`` (a ``utils.renderer.Depth_Renderer``) -- the
    inverse-depth image of the same mesh and camera (:456-460).  -> the batch's loss inputs as fp32 device tensors plus ``opt_vertices``,
    ``opt_sub_vertices``, ``opt_temp_vertices``, ``opt_joints``, ``opt_cam_t`` (and ``iuv_image_gt``, ``depth_image_gt``)."""
    keys = ('pose', 'betas', 'pose_3d', 'has_smpl', 'has_pose_3d', 'keypoints', 'keypoints_world', 'orig_shape', 'bbox_width', 'bbox_height', 'focal')
    for k in keys:
        if k in input_batch and not input_batch[k].is_cuda:
            raise RuntimeError('whmr_amd runs on a HIP device only (no CPU fallback)')
    t = {k: _f32(input_batch[k]) for k in keys if k in input_batch}
    reg = model.regressor[0]
    B = t['pose'].shape[0]
    rot = L.rot_to_mat(t['pose'].reshape(-1, 3), L.RODRIGUES).view(B, 24, 3, 3)        # smpl(pose2rot=True), trainer.py:420
    out = reg.smpl.run(t['betas'], rot)
    c = downsample_csr(reg.Dmap0, reg.Dmap1, model.__dict__.setdefault('_target_cache', {}))
    sub = L.csr_apply3(c['d0'], out.vertices, reg.Dmap0.shape[0])
    t.update(opt_vertices=out.vertices, opt_joints=out.joints, opt_sub_vertices=sub,
             opt_temp_vertices=L.csr_apply3(c['d1'], sub, reg.Dmap1.shape[0]))
    kp = t['keypoints'].clone()
    kp[:, :, :-1] = 0.5 * img_res * (kp[:, :, :-1] + 1)                                 # trainer.py:430-431
    t['opt_cam_t'] = estimate_translation(out.joints, kp, focal_length=FOCAL_LENGTH, img_size=[cfg.IMG_RES.WIDTH, cfg.IMG_RES.HEIGHT])
    if iuv_maker is not None or depth_maker is not None:
        cam = gt_camera_from_translation(t['opt_cam_t'], focal_length=FOCAL_LENGTH)
        crop = cfg.MODEL.PyMAF.BACKBONE == 'vitpose'
        if iuv_maker is not None:
            t['iuv_image_gt'], _ = render_iuv_targets(iuv_maker, out.vertices, cam, vitpose_crop=crop, maps=False)
        if depth_maker is not None:
            t['depth_image_gt'] = render_depth_target(depth_maker, out.vertices, cam, vitpose_crop=crop)
    return t
