"""The training objective of core/trainer.py:498-609 restated in torch, in the mask-multiplication form (no boolean gather, no host read), for any
dtype and device: float64 on the CPU is the reference of the fused node's tests, float32 is the "same arithmetic, other summation order" yardstick
and the launch-count baseline of tools/loss_timing.py.  Written from the cited lines; tests/golden/whmr_losses.npz pins it to the reference's own
methods (tests/golden/make_golden_losses.py)."""
import torch

FIELDS = ('rotmat', 'shape', 'kp_3d', 'verts', 'sub_verts', 'temp_verts', 'cam', 'kp_2d', 'kp_2d_w', 'focal')
TARGETS = ('gt_pose', 'gt_betas', 'pose_3d', 'has_smpl', 'has_pose_3d', 'gt_verts', 'gt_sub_verts', 'gt_temp_verts', 'gt_kp_2d', 'gt_kp_2d_w',
           'orig_shape', 'bbox_width', 'bbox_height', 'gt_focal')
DEFAULT_W = {'w_pose': 60.0, 'w_shape': 0.06, 'w_kp3d': 300.0, 'w_vert': 15.0, 'w_kp2d': 0.0, 'w_focal': 1e-6, 'w_openpose': 0.0, 'w_gt': 1.0}
ALL_ON_W = dict(DEFAULT_W, w_kp2d=300.0, w_openpose=0.5)


def batch_rodrigues(theta):
    """utils/geometry.py:14-51"""
    angle = torch.norm(theta + 1e-8, p=2, dim=1, keepdim=True)
    n = theta / angle
    q = torch.cat([torch.cos(angle * 0.5), torch.sin(angle * 0.5) * n], dim=1)
    q = q / q.norm(p=2, dim=1, keepdim=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    return torch.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz, 2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                        2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], dim=1).view(-1, 3, 3)


def _masked_mean(x, mask):
    """mean of x over the samples with mask != 0 (x[mask].mean() of the reference), 0 when there is none: the masked-out samples are multiplied by
    0 and the count is clamped, so nothing is gathered and nothing is read on the host"""
    m = mask.to(x.dtype)
    per = x.reshape(x.shape[0], -1)
    return (per * m[:, None]).sum() / (m.sum().clamp(min=1.0) * per.shape[1])


def smpl_losses(rotmat, shape, gt_pose, gt_betas, has_smpl):
    """trainer.py:242-253 -> (loss_regr_pose, loss_regr_betas), unweighted"""
    R = batch_rodrigues(gt_pose.reshape(-1, 3)).view(-1, 24, 3, 3)
    return _masked_mean((rotmat - R) ** 2, has_smpl), _masked_mean((shape - gt_betas) ** 2, has_smpl)


def keypoint_3d_loss(kp_3d, pose_3d, has_pose_3d):
    """trainer.py:214-231"""
    p, conf, g = kp_3d[:, 25:, :], pose_3d[:, :, 3:], pose_3d[:, :, :3]
    g = g - ((g[:, 2, :] + g[:, 3, :]) / 2)[:, None, :]
    p = p - ((p[:, 2, :] + p[:, 3, :]) / 2)[:, None, :]
    return _masked_mean(conf * (p - g) ** 2, has_pose_3d)


def shape_loss(verts, gt_verts, has_smpl):
    """trainer.py:233-240"""
    return _masked_mean((verts - gt_verts).abs(), has_smpl)


def keypoint_loss(kp_2d, gt, w_openpose, w_gt):
    """trainer.py:203-212 -> [B, 49, 2], not reduced"""
    conf = gt[:, :, -1:].clone()
    conf[:, :25] = conf[:, :25] * w_openpose
    conf[:, 25:] = conf[:, 25:] * w_gt
    return conf * (kp_2d - gt[:, :, :-1]) ** 2


def world_scale(orig_shape, bbox_width, bbox_height):
    """trainer.py:501-506 -> [B, 1, 2]"""
    return torch.stack([orig_shape[:, 1] / bbox_width, orig_shape[:, 0] / bbox_height], dim=1)[:, None, :]


def loss_dict(preds, tgt, w):
    """trainer.py:508-587: preds = three dicts of FIELDS (None / absent = term off), tgt = dict of TARGETS, w = weights as DEFAULT_W -> {key: 0-dim}"""
    out = {}
    for l, p in enumerate(preds, 1):
        lp, lb = smpl_losses(p['rotmat'], p['shape'], tgt['gt_pose'], tgt['gt_betas'], tgt['has_smpl'])
        out['loss_regr_pose_%d' % l] = lp * w['w_pose']
        out['loss_regr_betas_%d' % l] = lb * w['w_shape']
        if p.get('kp_2d') is not None:
            out['loss_keypoints_%d' % l] = keypoint_loss(p['kp_2d'], tgt['gt_kp_2d'], w['w_openpose'], w['w_gt']).mean() * w['w_kp2d']
            out['loss_keypoints_world_%d' % l] = (keypoint_loss(p['kp_2d_w'], tgt['gt_kp_2d_w'], w['w_openpose'], w['w_gt'])
                                                  * world_scale(tgt['orig_shape'], tgt['bbox_width'], tgt['bbox_height'])).mean() * w['w_kp2d']
        if p.get('focal') is not None:
            out['loss_focal_length_%d' % l] = ((p['focal'] - tgt['gt_focal']) ** 2).mean() * w['w_focal']               # :566-569
        out['loss_keypoints_3d_%d' % l] = keypoint_3d_loss(p['kp_3d'], tgt['pose_3d'], tgt['has_pose_3d']) * w['w_kp3d']
        if p.get('verts') is not None:
            for k, name in (('verts', 'loss_shape'), ('sub_verts', 'loss_shape_sub'), ('temp_verts', 'loss_shape_temp')):
                out['%s_%d' % (name, l)] = shape_loss(p[k], tgt['gt_' + k], tgt['has_smpl']) * w['w_vert']
        out['loss_cam_%d' % l] = (torch.exp(-p['cam'][:, 0] * 10) ** 2).mean()                                         # :586
    return out


def make_case(B, V, seed, has_smpl, has_pose_3d, all_on=False, dtype=torch.float64):
    """seeded inputs of the objective: (preds, tgt).  V = (V, V_sub, V_temp); the vertex terms belong to the last stage only (trainer.py:576);
    all_on adds the 2-D keypoint and focal-length inputs.  Magnitudes are those of a training step (metres, normalised image coordinates)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    tgt = {'gt_pose': rn(B, 72) * 0.6, 'gt_betas': rn(B, 10), 'pose_3d': torch.cat([rn(B, 24, 3) * 0.4, (ru(B, 24, 1) > 0.25).double() * ru(B, 24, 1)], -1),
           'has_smpl': torch.as_tensor(has_smpl, dtype=torch.float64), 'has_pose_3d': torch.as_tensor(has_pose_3d, dtype=torch.float64),
           'gt_verts': rn(B, V[0], 3) * 0.4, 'gt_sub_verts': rn(B, V[1], 3) * 0.4, 'gt_temp_verts': rn(B, V[2], 3) * 0.4}
    if all_on:
        tgt.update(gt_kp_2d=torch.cat([rn(B, 49, 2) * 0.5, (ru(B, 49, 1) > 0.3).double() * ru(B, 49, 1)], -1),
                   gt_kp_2d_w=torch.cat([rn(B, 49, 2) * 0.5, (ru(B, 49, 1) > 0.3).double() * ru(B, 49, 1)], -1),
                   orig_shape=torch.stack([ru(B) * 800 + 400, ru(B) * 1200 + 600], 1).floor(), bbox_width=ru(B) * 300 + 80, bbox_height=ru(B) * 400 + 120,
                   gt_focal=ru(B) * 1500 + 800)
    assert tgt['has_smpl'].shape == (B,) and tgt['has_pose_3d'].shape == (B,)
    R = batch_rodrigues(tgt['gt_pose'].reshape(-1, 3)).view(B, 24, 3, 3)
    preds = []
    for l in range(3):
        p = {'rotmat': R + rn(B, 24, 3, 3) * 0.2, 'shape': tgt['gt_betas'] + rn(B, 10) * 0.5, 'cam': torch.cat([ru(B, 1) * 0.3 - 0.05, rn(B, 2) * 0.1], 1),
             'kp_3d': rn(B, 49, 3) * 0.4}
        if l == 2:
            for k in ('verts', 'sub_verts', 'temp_verts'):
                p[k] = tgt['gt_' + k] + rn(*tgt['gt_' + k].shape) * 0.05
        if all_on:
            p.update(kp_2d=tgt['gt_kp_2d'][..., :2] + rn(B, 49, 2) * 0.1, kp_2d_w=tgt['gt_kp_2d_w'][..., :2] + rn(B, 49, 2) * 0.1,
                     focal=tgt['gt_focal'] + rn(B) * 200)
        preds.append(p)
    cast = lambda d: {k: v.to(dtype) for k, v in d.items()}
    return [cast(p) for p in preds], cast(tgt)


def to(preds, tgt, device=None, dtype=None, requires_grad=False):
    """copies of a case on another device / in another dtype; requires_grad makes the predictions leaves"""
    mv = lambda v: v.detach().to(device=device, dtype=dtype).clone()
    return [{k: mv(v).requires_grad_(requires_grad) for k, v in p.items()} for p in preds], {k: mv(v) for k, v in tgt.items()}
