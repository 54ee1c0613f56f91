"""What cfg.MODEL.PyMAF.DEPTH_SUPV_ON costs in the batch-64 training step (bf16 numerics), measured on one box in one process:

  * the whole step (forward, targets rendered from the stage-3 mesh, the objective's stand-in + the dense-correspondence terms, backward) with the
    flag off and on, ALTERNATING in rounds (off, on, off, on, ...) so that clock and thermal drift hit both alike; median over the rounds;
  * the launches the flag adds, each alone: the depth rasteriser (whmr_depth_rasterize, three launches), the loss forward (whmr_depth_loss, two
    launches) and the loss backward (whmr_depth_loss_bwd, one launch into column 90 of the gradient buffer);
  * the head convolution's launch count is unchanged by construction (the depth head is output channel 90 of the IUV head's GEMM, padded to 128
    columns either way): no separate figure exists for it.

    python tools/depth_supv_timing.py [rounds] [steps per round]        -> profiles/depth_supv_timing.txt
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from whmr_amd import _lib as L
from whmr_amd.core.cfgs import cfg
from whmr_amd.models import whmr_net
from whmr_amd.train.aux_supervision import AuxLossFn, IUVLossFn, render_depth_target, render_iuv_targets
from whmr_amd.utils import synth
from whmr_amd.utils.renderer import Depth_Renderer, IUV_Renderer

LOSS_KEYS = ('rotmat', 'pred_shape', 'pred_cam', 'kp_2d', 'kp_2d_w', 'kp_3d', 'verts', 'sub_verts', 'temp_verts')
B = 64


def make_model(assets, sd, depth, dev):
    cfg.MODEL.PyMAF.DEPTH_SUPV_ON = depth
    m = whmr_net(None, assets=assets, numerics='bf16')
    m.load_state_dict(sd, strict=False)
    m = m.to(dev).train()
    for name, p in m.named_parameters():
        if name.startswith(('cam_model', 'global_orient')):
            p.requires_grad_(False)
    return m, [p for p in m.parameters() if p.requires_grad]


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    dev = torch.device('cuda:0')
    assets = synth.make_assets(0)
    sd = synth.make_state_dict(0, assets, with_cam_model=False)
    tables = synth.make_densepose_tables(0, assets)
    iuv_maker = IUV_Renderer(orig_size=(256, 256), output_size=(128, 128), dp=tables)
    # the synthetic assets carry no SMPL connectivity: the DensePose-sized face table restricted to the 6890 SMPL vertices stands in for it
    faces = tables['faces'].long()
    faces = faces[(faces < 6890).all(1)].to(torch.int32)
    depth_maker = Depth_Renderer(orig_size=(256, 256), output_size=(128, 128), faces=faces)
    gt_cam = torch.tensor([[0.9, 0.0, 0.0]], device=dev).expand(B, -1).contiguous()
    has_smpl = torch.ones(B, device=dev)
    inp = synth.make_inputs(B, 0)
    d = {k: inp[k].to(dev) for k in ('x', 'center', 'scale', 'bbox_height', 'orig_shape', 'bbox_info')}
    w = float(cfg.LOSS.POINT_REGRESSION_WEIGHTS)
    old = cfg.MODEL.PyMAF.DEPTH_SUPV_ON
    try:
        models = {flag: make_model(assets, sd, flag, dev) for flag in (False, True)}

        def step(flag):
            cfg.MODEL.PyMAF.DEPTH_SUPV_ON = flag
            m, params = models[flag]
            for p in params:
                p.grad = None
            out, _ = m(d['x'], None, d['center'], d['scale'], d['bbox_height'], d['orig_shape'], d['bbox_info'], is_train=True)
            loss = sum(out['smpl_out'][l][k].float().pow(2).mean() for l in range(1, 4) for k in LOSS_KEYS)
            mesh = out['smpl_out'][-1]['verts'].detach()
            img, _ = render_iuv_targets(iuv_maker, mesh, gt_cam, maps=False)
            if flag:
                dimg = render_depth_target(depth_maker, mesh, gt_cam)
                loss = loss + AuxLossFn.apply(out['dpth_out'][0].nhwc, img, dimg, has_smpl, w).sum()
            else:
                loss = loss + IUVLossFn.apply(out['dp_out'][0].nhwc, img, w).sum()
            loss.backward()
            return loss, mesh

        for flag in (False, True):
            for _ in range(3):
                step(flag)
        torch.cuda.synchronize()
        per = {False: [], True: []}
        for _ in range(rounds):
            for flag in (False, True):
                per[flag].append(events_ms(lambda: step(flag), steps))
        _, mesh = step(True)
        out, _ = models[True][0](d['x'], None, d['center'], d['scale'], d['bbox_height'], d['orig_shape'], d['bbox_info'], is_train=True)
        y91 = out['dpth_out'][0].nhwc.detach()
        dimg = render_depth_target(depth_maker, mesh, gt_cam)
        covered = (dimg > 0).float().mean().item()
        g = torch.ones(1, device=dev)
        dyp = torch.zeros(B * 128 * 96, y91.stride(2), dtype=y91.dtype, device=dev)
        for fn in (lambda: depth_maker.verts2depthimg(mesh, gt_cam), lambda: L.depth_loss(y91, 90, dimg, has_smpl, w),
                   lambda: L.depth_loss_bwd(y91, 90, dimg, has_smpl, w, g, dyp)):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t_raster = events_ms(lambda: depth_maker.verts2depthimg(mesh, gt_cam), 50)
        t_fwd = events_ms(lambda: L.depth_loss(y91, 90, dimg, has_smpl, w), 50)
        t_bwd = events_ms(lambda: L.depth_loss_bwd(y91, 90, dimg, has_smpl, w, g, dyp), 50)
    finally:
        cfg.MODEL.PyMAF.DEPTH_SUPV_ON = old
    off, on = statistics.median(per[False]), statistics.median(per[True])
    lines = ['# python tools/depth_supv_timing.py %d %d   (one MI355X, one process, flag off / on alternating per round)' % (rounds, steps),
             'torch %s, %s' % (torch.__version__, torch.cuda.get_device_name(0)),
             'training step, batch %d, bf16, eager (forward + rendered targets + losses + backward, no optimizer), ms per step, %d rounds x %d steps:' % (B, rounds, steps),
             '  DEPTH_SUPV_ON off: median %.3f  (rounds: %s)' % (off, ' '.join('%.3f' % t for t in per[False])),
             '  DEPTH_SUPV_ON on:  median %.3f  (rounds: %s)' % (on, ' '.join('%.3f' % t for t in per[True])),
             '  difference of the medians: %+.3f ms (%+.2f %%); spread of one configuration over the rounds: off %.3f, on %.3f ms'
             % (on - off, 100.0 * (on - off) / off, max(per[False]) - min(per[False]), max(per[True]) - min(per[True])),
             'the launches the flag adds, each alone (HIP events over 50 calls, wrapper allocations included):',
             '  depth rasteriser, %d faces on 6890 vertices, %d x 128 x 128 (3 launches): %.1f us   (%.3f of the pixels covered)' % (faces.shape[0], B, t_raster * 1e3, covered),
             '  loss forward, column 90 of [%d, %d] bf16 (2 launches): %.1f us' % (B * 128 * 96, y91.stride(2), t_fwd * 1e3),
             '  loss backward into column 90 of the gradient buffer (1 launch): %.1f us' % (t_bwd * 1e3),
             'head convolution: one GEMM launch forward, the same data- and weight-gradient launches backward, with the flag off and on (91 of 128 padded columns used instead of 90)']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'depth_supv_timing.txt'), 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
