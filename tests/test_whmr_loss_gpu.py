"""The fused training objective (csrc/whmr_loss.hip through whmr_amd.train.objective) on the MI355X against the float64 restatement of
core/trainer.py:498-609 (tests/whmr_loss_reference.py, pinned to the reference's own methods by tests/golden/whmr_losses.npz)."""
import functools
import types

import pytest
import torch

import whmr_loss_reference as WR

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-5            # |loss - ref| <= LOSS_TOL * max(1, |ref|): the project's loss bound (tests/golden/make_golden_train.py)
GRAD_TOL = 1e-5            # max |g - ref| <= GRAD_TOL * max |ref| per gradient tensor
MASKED = ('loss_regr_pose', 'loss_regr_betas', 'loss_keypoints_3d', 'loss_shape', 'loss_shape_sub', 'loss_shape_temp')
FULL, SMALL = (6890, 1723, 431), (37, 11, 5)
OPTIONS = types.SimpleNamespace(openpose_train_weight=0.5, gt_train_weight=1.0)


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


class config:
    """cfg with every optional term on (KP_2D_W = 300, FOCAL_SUPV_ON), restored on exit"""

    def __init__(self, all_on):
        self.all_on = all_on

    def __enter__(self):
        from whmr_amd.core.cfgs import cfg
        self.old = (cfg.LOSS.KP_2D_W, cfg.MODEL.PyMAF.FOCAL_SUPV_ON)
        if self.all_on:
            cfg.LOSS.KP_2D_W, cfg.MODEL.PyMAF.FOCAL_SUPV_ON = 300.0, True
        return self

    def __exit__(self, *exc):
        from whmr_amd.core.cfgs import cfg
        cfg.LOSS.KP_2D_W, cfg.MODEL.PyMAF.FOCAL_SUPV_ON = self.old


@functools.lru_cache(maxsize=None)
def _case(B, V, all_on, has_smpl, has_pose_3d, seed=0):
    """fp32 inputs and their float64 reference (values + gradients by autograd), computed once and shared"""
    preds, tgt = WR.make_case(B, V, seed, list(has_smpl), list(has_pose_3d), all_on=all_on, dtype=torch.float32)
    p64, t64 = WR.to(preds, tgt, dtype=torch.float64, requires_grad=True)
    ref = WR.loss_dict(p64, t64, WR.ALL_ON_W if all_on else WR.DEFAULT_W)
    torch.stack(list(ref.values())).sum().backward()
    return preds, tgt, {k: v.detach() for k, v in ref.items()}, [{k: v.grad for k, v in p.items()} for p in p64]


def _on_device(preds, tgt, dev):
    """leaf tensors on the device; theta = [cam | shape | pose] as the model concatenates it, so that compute_losses reads the two as column slices"""
    pd, td = WR.to(preds, tgt, device=dev, requires_grad=True)
    B = td['gt_pose'].shape[0]
    smpl_out = [None]
    for p in pd:
        d = {k: v for k, v in p.items() if k not in ('shape', 'cam', 'focal')}
        d['theta'] = torch.cat([p['cam'], p['shape'], torch.zeros(B, 72, device=dev)], dim=1)
        d['focal_length'] = p.get('focal')
        smpl_out.append(d)
    batch = {'pose': td['gt_pose'], 'betas': td['gt_betas'], 'pose_3d': td['pose_3d'], 'has_smpl': td['has_smpl'],
             'has_pose_3d': td['has_pose_3d'].long(),                                   # int64 in the batch (datasets/train_batch.py)
             'opt_vertices': td['gt_verts'], 'opt_sub_vertices': td['gt_sub_verts'], 'opt_temp_vertices': td['gt_temp_verts']}
    if 'gt_kp_2d' in td:
        batch.update(keypoints=td['gt_kp_2d'], keypoints_world=td['gt_kp_2d_w'], orig_shape=td['orig_shape'].long(), bbox_width=td['bbox_width'],
                     bbox_height=td['bbox_height'], focal=td['gt_focal'])
    return pd, {'smpl_out': smpl_out, 'dp_out': []}, batch


def _run(preds, tgt, dev, all_on):
    """compute_losses + backward of the total -> (loss_dict, leaf predictions with .grad)"""
    from whmr_amd.train import compute_losses, total_loss
    pd, preds_dict, batch = _on_device(preds, tgt, dev)
    with config(all_on):
        d = compute_losses(preds_dict, batch, OPTIONS if all_on else None)
        total_loss(d).backward()
    return d, pd


def _compare(d, pd, ref, gref, what):
    assert list(d) == list(ref), (what, list(d), list(ref))
    worst_l = worst_g = 0.0
    for k, r in ref.items():
        v = d[k]
        assert v.dim() == 0 and v.dtype == torch.float32
        e = abs(v.item() - r.item()) / max(1.0, abs(r.item()))
        worst_l = max(worst_l, e)
        print('%s %-24s %.8g ref %.8g  err %.1e' % (what, k, v.item(), r.item(), e))
        assert e <= LOSS_TOL, (what, k, v.item(), r.item())
    for l, (p, g) in enumerate(zip(pd, gref), 1):
        for k, r in g.items():
            assert p[k].grad is not None and p[k].grad.shape == r.shape, (what, l, k)
            assert torch.isfinite(p[k].grad).all(), (what, l, k)
            if not r.any():
                assert not p[k].grad.any(), (what, l, k)
                continue
            e = _rel(p[k].grad.cpu(), r)
            worst_g = max(worst_g, e)
            print('%s stage %d d/d %-10s max %.3e  err %.1e' % (what, l, k, r.abs().max().item(), e))
            assert e <= GRAD_TOL, (what, l, k, e)
    print('%s: worst loss error %.1e, worst gradient error %.1e' % (what, worst_l, worst_g))


@pytest.mark.parametrize('all_on', [False, True], ids=['default', 'all_on'])
@pytest.mark.parametrize('V', [FULL, SMALL], ids=['smpl_mesh', 'tiny_mesh'])
def test_values_and_gradients_match_the_float64_restatement(dev, V, all_on):
    """B = 5, mixed masks; 6890 / 1723 / 431 vertices (103350 elements: 100 chunks + a tail) and 37 / 11 / 5 (terms smaller than one chunk); the
    default configuration (15 terms) and every optional term on (24).  Every figure is printed before it is asserted (pytest -s)."""
    preds, tgt, ref, gref = _case(5, V, all_on, (1, 0, 1, 1, 0), (0, 1, 1, 0, 1))
    d, pd = _run(preds, tgt, dev, all_on)
    assert len(d) == (24 if all_on else 15)
    _compare(d, pd, ref, gref, '%s %s' % (V[0], 'all-on' if all_on else 'default'))
    kp = pd[2]['kp_3d'].grad
    assert not kp[:, :25].any() and kp[:, 25:].any()                                 # rows 0-24 do not enter the loss (trainer.py:218)


@pytest.mark.parametrize('B,has_smpl,has_pose_3d', [(5, (0,) * 5, (0,) * 5), (5, (0, 0, 0, 1, 0), (0, 1, 0, 0, 0)), (1, (1,), (1,)), (1, (0,), (0,))],
                         ids=['none_valid', 'one_valid', 'B1', 'B1_none_valid'])
def test_empty_and_single_sample_masks(dev, B, has_smpl, has_pose_3d):
    """no valid sample: the masked terms are 0.0 exactly, their gradients all-zero and finite (no division by the zero count); one valid sample and
    B = 1 against the restatement"""
    preds, tgt, ref, gref = _case(B, SMALL, True, has_smpl, has_pose_3d, seed=3)
    d, pd = _run(preds, tgt, dev, True)
    _compare(d, pd, ref, gref, 'B %d masks %s' % (B, has_smpl))
    if not any(has_smpl):
        for k, v in d.items():
            if k.rsplit('_', 1)[0] in MASKED:
                assert v.item() == 0.0, k
        for p in pd:
            for k in ('rotmat', 'shape', 'kp_3d', 'verts', 'sub_verts', 'temp_verts'):
                if k in p:
                    assert torch.isfinite(p[k].grad).all() and not p[k].grad.any(), k
            assert p['cam'].grad[:, 0].abs().min() > 0 and p['kp_2d'].grad.any()      # the unmasked terms keep their gradients


def test_l1_gradient_is_zero_where_the_prediction_equals_the_target(dev):
    """sign(0) = 0 as torch's L1 backward (trainer.py:100, :238)"""
    preds, tgt, _, _ = _case(5, SMALL, False, (1, 0, 1, 1, 0), (0, 1, 1, 0, 1))
    preds = [dict(p) for p in preds]
    hit = torch.zeros(5, 37, 3, dtype=torch.bool)
    hit[0, 3], hit[2, ::5, 1], hit[3, 36, 2] = True, True, True
    preds[2]['verts'] = torch.where(hit, tgt['gt_verts'], preds[2]['verts'])
    d, pd = _run(preds, tgt, dev, False)
    g = pd[2]['verts'].grad.cpu()
    valid = tgt['has_smpl'].bool()[:, None, None].expand_as(hit)
    assert not g[hit].any() and (g[valid & ~hit] != 0).all() and not g[~valid].any()
    assert g.abs().max().item() == pytest.approx(15.0 / (3 * 37 * 3), rel=1e-6)          # VERT_W / (valid samples * elements per sample)


def test_two_calls_are_bit_identical(dev):
    preds, tgt, _, _ = _case(5, FULL, True, (1, 0, 1, 1, 0), (0, 1, 1, 0, 1))
    (d1, p1), (d2, p2) = _run(preds, tgt, dev, True), _run(preds, tgt, dev, True)
    assert all(torch.equal(d1[k], d2[k]) for k in d1)
    assert all(torch.equal(a[k].grad, b[k].grad) for a, b in zip(p1, p2) for k in a)


def test_node_replays_from_a_captured_graph_with_other_masks(dev):
    """forward + backward of the node captured with torch.cuda.graph on one stream; the static inputs are then refilled -- other values, masks with
    another valid count, an all-zero mask -- and the replay equals an eager call on the same contents bit for bit: the valid counts never visit
    the host"""
    from whmr_amd import _lib as L
    from whmr_amd.train import WHMRLossFn
    n = len(L.LOSS_FIELDS)
    fills = [_case(5, SMALL, True, hs, h3, seed=s)[:2] for hs, h3, s in (((1, 0, 1, 1, 0), (0, 1, 1, 0, 1), 0), ((1, 1, 1, 1, 0), (1, 0, 0, 0, 0), 4),
                                                                           ((0,) * 5, (0,) * 5, 5), ((1,) * 5, (1,) * 5, 6))]
    pd, td = WR.to(*fills[0], device=dev, requires_grad=True)
    flat = [p.get(k) for p in pd for k in L.LOSS_FIELDS]
    leaves = [t for t in flat if t is not None]
    cot = torch.linspace(0.5, 1.5, L.LOSS_STAGES * n, device=dev)

    def node():
        losses = WHMRLossFn.apply(td, WR.ALL_ON_W, *flat)
        return losses, torch.autograd.grad(losses, leaves, cot)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        node()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        losses, grads = node()
    for i, (preds, tgt) in enumerate(fills[1:] + fills[:1]):
        with torch.no_grad():
            for p, src in zip(pd, preds):
                for k in p:
                    p[k].copy_(src[k])
            for k in td:
                td[k].copy_(tgt[k])
        graph.replay()
        torch.cuda.synchronize()
        got_l, got_g = losses.clone(), [g.clone() for g in grads]
        want_l, want_g = node()
        assert torch.equal(got_l, want_l), (i, got_l, want_l)
        assert all(torch.equal(a, b) for a, b in zip(got_g, want_g)), i
        if i == 1:                                                                   # the all-zero masks
            assert not got_l.view(L.LOSS_STAGES, n)[:, :6].any() and torch.isfinite(torch.cat([g.reshape(-1) for g in got_g])).all()
        elif i == 0:
            assert got_l.view(L.LOSS_STAGES, n)[:, :3].all()


def _expected_keys(all_on):
    keys = []
    for l in (1, 2, 3):                                                              # core/trainer.py:538-587, in the order the reference fills loss_dict
        keys += ['loss_regr_pose_%d' % l, 'loss_regr_betas_%d' % l]
        keys += ['loss_keypoints_%d' % l, 'loss_keypoints_world_%d' % l, 'loss_focal_length_%d' % l] if all_on else []
        keys += ['loss_keypoints_3d_%d' % l]
        keys += ['loss_shape_3', 'loss_shape_sub_3', 'loss_shape_temp_3'] if l == 3 else []
        keys += ['loss_cam_%d' % l]
    return keys


@pytest.mark.parametrize('all_on', [False, True], ids=['default', 'all_on'])
def test_key_set_is_the_references(dev, all_on):
    """15 / 24 smpl_out keys, plus loss_U-1 ... loss_segAnn-1 (core/trainer.py:484-487) when the rendered image is among the targets"""
    from whmr_amd.train import compute_losses, total_loss
    from whmr_amd.train.aux_supervision import IUVHeadOutput
    preds, tgt, _, _ = _case(5, SMALL, all_on, (1, 0, 1, 1, 0), (0, 1, 1, 0, 1))
    pd, preds_dict, batch = _on_device(preds, tgt, dev)
    g = torch.Generator().manual_seed(0)
    with config(all_on):
        d = compute_losses(preds_dict, batch, OPTIONS)
        assert list(d) == _expected_keys(all_on) and len(d) == (24 if all_on else 15)
        preds_dict['dp_out'] = [IUVHeadOutput(torch.randn(5, 8, 6, 90, generator=g).to(dev).requires_grad_(True))]
        iuv = torch.rand(5, 3, 8, 6, generator=g)
        iuv[:, 0] = torch.randint(0, 25, (5, 8, 6), generator=g) / 24.0
        d2 = compute_losses(preds_dict, dict(batch, iuv_image_gt=iuv.to(dev)), OPTIONS)
    iuv_keys = ['loss_U-1', 'loss_V-1', 'loss_IndexUV-1', 'loss_segAnn-1']
    assert list(d2) == iuv_keys + _expected_keys(all_on)
    assert all(v.dim() == 0 and torch.isfinite(v) for v in d2.values()) and all(d2[k].item() > 0 for k in iuv_keys)
    tot, ref = total_loss(d2), torch.stack(list(d2.values())).double().sum()
    assert abs(tot.item() - ref.item()) <= LOSS_TOL * max(1.0, abs(ref.item()))
    tot.backward()
    assert preds_dict['dp_out'][0].nhwc.grad is not None and pd[0]['rotmat'].grad is not None


def test_parameter_gradients_through_the_model_match_the_float32_restatement(dev, assets, state_dict):
    """the smallest training model of tests/test_train_gpu.py (synthetic SMPL, fp32, B = 2): total_loss(compute_losses(...)).backward() against the
    float32 torch restatement applied to the same preds_dict -- same graph below the loss, so the parameter gradients agree to that file's bound
    for two fp32 evaluations of one step on the device (1e-4 of each tensor's largest magnitude)"""
    from oracle import synth
    from whmr_amd.models import whmr_net
    from whmr_amd.train import compute_losses, total_loss
    m = whmr_net(None, assets=assets, numerics='fp32')
    res = m.load_state_dict(state_dict, strict=False)
    assert not res.unexpected_keys
    m = m.to(dev).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m.feature_extractor.backbone.drop_path_rate = 0.0
    inp = synth.make_inputs(2, 0)
    x = {k: inp[k].to(dev) for k in ('x', 'center', 'scale', 'bbox_height', 'orig_shape', 'bbox_info')}
    _, tgt = WR.make_case(2, FULL, 7, [1, 0], [1, 1], dtype=torch.float32)
    tgt = {k: v.to(dev) for k, v in tgt.items()}
    batch = {'pose': tgt['gt_pose'], 'betas': tgt['gt_betas'], 'pose_3d': tgt['pose_3d'], 'has_smpl': tgt['has_smpl'], 'has_pose_3d': tgt['has_pose_3d'],
             'opt_vertices': tgt['gt_verts'], 'opt_sub_vertices': tgt['gt_sub_verts'], 'opt_temp_vertices': tgt['gt_temp_verts']}
    params = dict(m.named_parameters())

    def step(fused):
        for p in params.values():
            p.grad = None
        out, _ = m(x['x'], None, x['center'], x['scale'], x['bbox_height'], x['orig_shape'], x['bbox_info'], is_train=True)
        if fused:
            d = compute_losses(out, batch)
            total = total_loss(d)
        else:
            preds = [{'rotmat': s['rotmat'], 'shape': s['theta'][:, 3:13], 'cam': s['theta'][:, :3], 'kp_3d': s['kp_3d']} for s in out['smpl_out'][1:]]
            preds[2].update({k: out['smpl_out'][3][k] for k in ('verts', 'sub_verts', 'temp_verts')})
            d = WR.loss_dict(preds, tgt, WR.DEFAULT_W)
            total = torch.stack(list(d.values())).sum()
        total.backward()
        return {k: v.detach().clone() for k, v in d.items()}, {k: p.grad.clone() for k, p in params.items() if p.grad is not None}

    d_ref, g_ref = step(False)
    d_hip, g_hip = step(True)
    assert list(d_hip) == list(d_ref) and len(d_hip) == 15
    for k in d_ref:
        assert abs(d_hip[k].item() - d_ref[k].item()) <= LOSS_TOL * max(1.0, abs(d_ref[k].item())), (k, d_hip[k].item(), d_ref[k].item())
    assert set(g_hip) == set(g_ref) and len(g_ref) > 100
    worst = max((_rel(g_hip[k], g_ref[k]), k) for k in g_ref if g_ref[k].abs().max() > 1e-8)
    print('parameter gradients, fused node vs float32 restatement: worst max-rel %.2e (%s) over %d tensors' % (worst + (len(g_ref),)))
    assert worst[0] < 1e-4, worst


def test_build_targets_matches_the_cpu_oracle(dev, assets, state_dict):
    """core/trainer.py:413-436 at B = 2: SMPL of the ground-truth parameters and the fitted translation against oracle.smpl /
    oracle.geometry.estimate_translation, the two down-samplings against the dense products -- each at the bound the kernel's own test uses (1e-5)"""
    from oracle import geometry as OG
    from oracle import smpl as OS
    from whmr_amd.models import whmr_net
    from whmr_amd.train import build_targets
    m = whmr_net(None, assets=assets, numerics='fp32')
    m.load_state_dict(state_dict, strict=False)
    m = m.to(dev)
    g = torch.Generator().manual_seed(2)
    pose, betas = torch.randn(2, 72, generator=g) * 0.4, torch.randn(2, 10, generator=g) * 0.5
    v_ref, j_ref = OS.smpl_forward(betas, OG.batch_rodrigues(pose.reshape(-1, 3)).view(2, 24, 3, 3), assets['smpl'])
    cam = j_ref + torch.tensor([[0.1, -0.2, 5.0], [-0.3, 0.2, 8.0]])[:, None]
    px = 1000.0 * cam[..., :2] / cam[..., 2:] + 128.0 + torch.randn(2, 49, 2, generator=g)
    conf = (torch.rand(2, 49, 1, generator=g) > 0.3).float() * torch.rand(2, 49, 1, generator=g)
    batch = {'pose': pose, 'betas': betas, 'keypoints': torch.cat([px / 112.0 - 1.0, conf], -1), 'has_smpl': torch.ones(2),
             'has_pose_3d': torch.tensor([1, 0]), 'pose_3d': torch.zeros(2, 24, 4)}
    t = build_targets(m, {k: v.to(dev) for k, v in batch.items()})
    assert t['opt_vertices'].shape == (2, 6890, 3) and t['opt_joints'].shape == (2, 49, 3) and not t['opt_vertices'].requires_grad
    assert t['has_pose_3d'].dtype == torch.float32 and 'iuv_image_gt' not in t
    assert _rel(t['opt_vertices'].cpu(), v_ref) < 1e-5 and _rel(t['opt_joints'].cpu(), j_ref) < 1e-5
    sub = torch.matmul(assets['Dmap0'].double(), t['opt_vertices'].cpu().double())
    assert _rel(t['opt_sub_vertices'].cpu(), sub) < 1e-5
    assert _rel(t['opt_temp_vertices'].cpu(), torch.matmul(assets['Dmap1'].double(), t['opt_sub_vertices'].cpu().double())) < 1e-5
    kp_px = torch.cat([0.5 * 224 * (batch['keypoints'][..., :2] + 1), conf], -1)
    et = OG.estimate_translation(t['opt_joints'].cpu(), kp_px, 1000., (256., 256.))
    assert _rel(t['opt_cam_t'].cpu(), et) < 1e-5 and (t['opt_cam_t'].cpu()[:, 2] - torch.tensor([5.0, 8.0])).abs().max() < 0.5
