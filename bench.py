"""Benchmark of the W-HMR hot path on MI355X.  Contract: see the task brief / DESIGN.md "Measurement".

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload vit224|vit256x192|vitl256x192|whmr|whmr_train] [--dump-outputs DIR] [--full [--no-cpu] ...]

A step = one forward of the hot path over one batch of 64 synthetic crops per GPU (inputs resident in HBM).
N=1 default workload = BASELINE.json configs[1]: ViT-B/16 backbone only, 224x224, batch 64, bf16 MFMA.
A plain run sets up, warms up, times the steps, writes --dump-outputs and prints its line: nothing else.  `--full` adds what runs after the
timed region: the instrumented step (roofline), the clock probe and the MFMA / HBM ceilings, CPU baselines, parity against the CPU oracle, the
whmr HBM rows and fp32 leg, and the default run's secondary legs; --no-cpu / --no-parity / --no-ceilings / --no-secondary trim a --full run.
`--gpus N` with N > 1 and no WORLD_SIZE in the environment: this process is only a LAUNCHER -- it never touches the GPU, starts
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 bench.py ...` as a CHILD process (never an
exec), relays rank 0's JSON line and exits with the child's return code.  Under torch.distributed.run (WORLD_SIZE set) it is one rank
per GPU over RCCL (reference: one process per GPU + NCCL init, train.py:26-33; DDP wrap core/trainer.py:70-95).  The forward workloads shard
by image with no data-path collective (replicas, weak scaling): only the timing barrier / max-reduce / rank count use the communicator;
`whmr_train` exchanges gradients (GradReducer) and BatchNorm buffers (broadcast_buffers) every step.
`--dryrun-cpu` (tests only): gloo + CPU tensors and a stand-in step, to exercise launcher / rank bookkeeping / reducer without a GPU;
its line says "data": "dryrun" and is not a measurement.
Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

VIT_FLOP_PER_IMG = {'vit224': 34.94e9, 'vit256x192': 34.20e9, 'vitl256x192': 119.9e9, 'whmr': 34.20e9 + 9.26e9 + 1.98e9,
                    'whmr_train': 3 * (34.20e9 + 9.26e9 + 1.98e9 + 5.10e9)}        # + IUV head: 4 3x3 convs, 90 channels on the 128x96 map
METRIC = {'vit224': 'images/sec ViT-B 224^2 batch-64 fwd', 'vit256x192': 'images/sec ViT-B 256x192 batch-64 fwd',
          'vitl256x192': 'images/sec ViT-L 256x192 fwd',
          'whmr': 'images/sec full W-HMR fwd (ViT-B + 3-iter MAF loop + cam_model + orientation) batch-64',
          'whmr_train': 'images/sec W-HMR train step (fwd + bwd + DP gradient all-reduce + Adam) batch-64 per GPU'}
WORKLOAD = {'vit224': 'ViT-B/16 backbone forward', 'vit256x192': 'ViT-B/16 backbone forward', 'vitl256x192': 'ViT-L/16 backbone forward',
            'whmr': 'full W-HMR forward (ViT-B + deconv pyramid + Tz head + 3-iteration MAF/regressor/SMPL loop + cam_model ResNet-50 + global orientation)',
            'whmr_train': 'W-HMR training step: WHMR.forward(is_train=True), synthetic loss on the supervised outputs, HIP backward, gradient buckets, fused Adam'}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--workload', default='vit224')
    ap.add_argument('--numerics', default='bf16')
    ap.add_argument('--full', action='store_true',
                    help='after the timed region, also measure what the headline does not need: roofline (instrumented step), clock and ceilings, CPU '
                         'baseline, parity, whmr HBM rows / fp32 leg, secondary legs (the --no-* options below trim these)')
    ap.add_argument('--no-cpu', action='store_true', help='--full: skip the CPU baseline leg')
    ap.add_argument('--no-parity', action='store_true', help='--full, whmr: skip the parity / fp32-mode leg (rocprofv3 runs: keeps the kernel table to the timed path)')
    ap.add_argument('--graph', action='store_true', help='whmr_train on one GPU: replay the whole step from one HIP graph')
    ap.add_argument('--loss', default='multi-tensor', choices=['multi-tensor', 'per-tensor'],
                    help='whmr_train: the synthetic L2 loss over the 27 supervised tensors as one concatenated weighted dot product (default: 4 launches) or as '
                         '27 x (pow, mean, add) torch expressions (~190 small launches per step on the critical stream)')
    ap.add_argument('--eager', action='store_true', help='whmr: time the eager module call instead of the HIP-graph replay (default: graph)')
    ap.add_argument('--serial', action='store_true', help='whmr: the eager call with the side streams folded into the main one (per-kernel durations without concurrency, for rocprofv3)')
    ap.add_argument('--full-x', default='hoisted', choices=('hoisted', 'per-crop', 'none'),
                    help='whmr (BASELINE configs[2]): full-frame input of cam_model -- one [1,3,600,800] frame shared by the batch (default), one frame per '
                         'crop [B,3,600,800] as demo/tester.py:161 replicates it, or none (camera rotation = identity given)')
    ap.add_argument('--ref-1gpu', type=float, default=None, help='images/sec of the same workload on 1 GPU: adds efficiency_vs_1gpu to the line')
    ap.add_argument('--master-port', type=int, default=None, help='rendezvous port of the self-launched ranks (default: a free port)')
    ap.add_argument('--dryrun-cpu', action='store_true', help='tests only: gloo/CPU stand-in step (launcher + rank bookkeeping), not a measurement')
    ap.add_argument('--batchnorm', default='auto', choices=('auto', 'sync', 'local'),
                    help='whmr_train: BatchNorm statistics of the four trained layers -- sync = over all ranks (the reference, core/trainer.py:83), local = per GPU; '
                         'auto = sync at world size > 1, local on one GPU (sync on one GPU runs the split kernels with a no-op exchange)')
    ap.add_argument('--wrap', default='reducer', choices=('reducer', 'ddp'),
                    help='whmr_train: how the data-parallel exchange is driven -- reducer = whmr_amd.parallel (GradReducer + convert_sync_batchnorm, default), '
                         'ddp = the reference\'s own two lines (core/trainer.py:83-86): nn.SyncBatchNorm.convert_sync_batchnorm(model) then '
                         'DistributedDataParallel(model, device_ids=[gpu], find_unused_parameters=True); needs a process group (torch.distributed.run)')
    ap.add_argument('--always-bucket', action='store_true',
                    help='whmr_train: pack and exchange the gradient buckets even at world size 1 (one-rank RCCL smoke of the reducer on a 1-GPU box)')
    ap.add_argument('--no-ceilings', action='store_true', help='--full: skip the attainable-ceiling / clock-probe kernels (rocprofv3 runs: keeps them out of the kernel table)')
    ap.add_argument('--no-secondary', action='store_true',
                    help='--full, default workload (vit224, 1 GPU): skip the short secondary legs (the same workload in bf16x3, BASELINE configs[2] whmr, configs[3] whmr_train)')
    ap.add_argument('--rank-timeout', type=float, default=1500.0,
                    help='launcher: seconds after which the child ranks are killed (process group) and the launcher exits 124; also the collective timeout')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step computed (rank 0) as DIR/<name>.npy in float32 / float64, at most 64 MB in all '
                         '(larger arrays as a fixed, seeded sample of their flat elements): two builds run with the same arguments compare output for output')
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    return args


def build_workload(args, dev):
    from whmr_amd.utils import synth                       # synthetic weights / inputs only (generator, not a compute path)
    from whmr_amd.models.pose_vit import ViT
    if args.workload in ('vit224', 'vit256x192', 'vitl256x192'):
        size = (224, 224) if args.workload == 'vit224' else (256, 192)
        large = args.workload == 'vitl256x192'                  # BASELINE configs[4] backbone: ViT-L/16, dim 1024, depth 24
        dim, depth, heads = (1024, 24, 16) if large else (768, 12, 12)
        sd = synth.make_vit_state(1, size, embed_dim=dim, depth=depth)
        m = ViT(img_size=size, patch_size=16, embed_dim=dim, depth=depth, num_heads=heads, ratio=1, mlp_ratio=4,
                qkv_bias=True, drop_path_rate=0.3, numerics=args.numerics)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).eval()
        x = synth.make_inputs(args.batch, 7, size)['x'].to(dev)
        return (lambda: m(x)), sd, x, size
    if args.workload == 'whmr':
        # BASELINE configs[2]: full W-HMR forward = ViT-B + deconvs + Tz head + 3-iteration MAF/regressor/SMPL loop + cam_model (ResNet-50 on
        # the full frame, whmr.py:509-522) + global orientation, 256x192 crops, 600x800 frames.  The step is replayed from ONE HIP
        # graph (GraphedForward); the instrumented roofline step and --eager run the plain module call.
        from whmr_amd.models import whmr_net
        from whmr_amd.graph import GraphedForward
        assets = synth.make_assets(0)
        sd = synth.make_state_dict(0, assets)
        m = whmr_net(None, assets=assets, numerics=args.numerics)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).eval()
        inp = {k: v.to(dev) for k, v in synth.make_inputs(args.batch, 7).items()}
        a = (inp['x'], None, inp['center'], inp['scale'], inp['bbox_height'], inp['orig_shape'], inp['bbox_info'])
        nf = {'hoisted': 1, 'per-crop': args.batch, 'none': 0}[args.full_x]
        kw = {}
        if nf:
            kw['full_x'] = torch.randn(nf, 3, 600, 800, generator=torch.Generator().manual_seed(11)).to(dev)
        args.full_x_note = {'hoisted': 'cam_model on ONE 600x800 frame shared by the batch (hoisted: identical result to the per-crop replication of demo/tester.py:161)',
                            'per-crop': 'cam_model on %d 600x800 frames (one per crop, as demo/tester.py:161 replicates the frame)' % args.batch,
                            'none': 'no full frame: camera rotation identity (cam_model not in the step)'}[args.full_x]
        args.parity_ctx = (m, sd, assets, inp, kw)
        eager = lambda: m(*a, **kw)

        def eager_serial():                     # the instrumented (per-launch event) step: the side streams folded back into the main one, so
            ov = (m.overlap_camera, m.overlap_tz)      # that an event pair brackets ITS launch alone, not whatever runs beside it
            m.overlap_camera = m.overlap_tz = False
            try:
                return m(*a, **kw)
            finally:
                m.overlap_camera, m.overlap_tz = ov
        args.eager_step = eager_serial
        if args.serial:
            return eager_serial, None, inp['x'], (256, 192)
        if args.eager:
            return eager, None, inp['x'], (256, 192)
        g = GraphedForward(m, *a, **kw)

        def graph_replay():
            g.graph.replay()
            return g.out                                    # the graph's static outputs, rewritten by every replay
        return graph_replay, None, inp['x'], (256, 192)
    if args.workload == 'whmr_train':
        # BASELINE configs[3] (train.py pymaf_net step, batch 64 per GPU, DP gradient all-reduce over RCCL): forward in training mode,
        # a synthetic L2 loss on the tensors core/trainer.py:500-600 supervises, backward through the HIP autograd nodes, bucketed
        # all-reduce(mean) of the gradients (whmr_amd.parallel.GradReducer), Adam update
        from whmr_amd.models import whmr_net
        from whmr_amd.parallel import GradReducer, broadcast_buffers
        assets = synth.make_assets(0)
        sd = synth.make_state_dict(0, assets, with_cam_model=False)
        m = whmr_net(None, assets=assets, numerics=args.numerics)
        m.load_state_dict(sd, strict=False)
        m = m.to(dev).train()
        for name, p in m.named_parameters():       # the camera-calibration ResNet-50 is frozen (pretrained, SURVEY 8e: 450 MB of gradients without it)
            if name.startswith('cam_model'):
                p.requires_grad_(False)
        named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
        params = [p for _, p in named]
        world = int(os.environ.get('WORLD_SIZE', '1'))
        use_graph = args.graph and world == 1
        # global_orient.* (and dp_head.* without AUX supervision) never receive a gradient -- the reference asks DDP for find_unused_parameters
        # (core/trainer.py:84-91); GradReducer drops them at its first finish().  The backbone is one autograd node, so its parameters get
        # their own buckets: the head buckets are exchanged while the ViT backward still runs.
        # BatchNorm: the reference converts every BatchNorm to SyncBatchNorm before DDP (core/trainer.py:83) -- at world size > 1 the four trained layers
        # take their statistics and gradients over ALL ranks (one packed fp64 all-reduce per layer and direction, whmr_amd.parallel.sync_bn)
        sync_bn = args.batchnorm == 'sync' or (args.batchnorm == 'auto' and world > 1)
        call = m
        if args.wrap == 'ddp':
            # the reference's own wrap, verbatim (core/trainer.py:83-86): torch swaps the BatchNorm modules for nn.SyncBatchNorm (whmr_amd honours them:
            # parallel/sync_bn.py::sync_of) and DDP's reducer exchanges the gradients the HIP autograd nodes hand to autograd; no GradReducer
            import torch.distributed as tdist
            from torch.nn.parallel import DistributedDataParallel
            if not tdist.is_initialized():
                raise SystemExit('bench.py --wrap ddp needs a process group: run under torch.distributed.run (one rank is enough)')
            m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(m)
            call = DistributedDataParallel(m, device_ids=[dev.index], find_unused_parameters=True)
            sync_bn, use_graph, red = True, False, None
        else:
            if sync_bn:
                from whmr_amd.parallel import convert_sync_batchnorm
                convert_sync_batchnorm(m, always=(world == 1))          # (world > 1: on its own communicator, beside the gradient buckets' -- ADVICE r5)
            red = None if use_graph else GradReducer(params, groups=[n.startswith('feature_extractor') for n, _ in named], always_bucket=args.always_bucket)
            if red is not None:
                red.attach(m.feature_extractor.backbone)          # the ViT node publishes its gradients block by block: buckets exchange under its backward
        args.sync_bn = sync_bn
        args.sync_group = getattr(m, 'whmr_sync_group', None)
        args.reducer = red
        rank = int(os.environ.get('RANK', '0'))
        inp = {k: v.to(dev) for k, v in synth.make_inputs(args.batch, 7 + rank).items()}
        a = (inp['x'], None, inp['center'], inp['scale'], inp['bbox_height'], inp['orig_shape'], inp['bbox_info'])
        keys = ('rotmat', 'pred_shape', 'pred_cam', 'kp_2d', 'kp_2d_w', 'kp_3d', 'verts', 'sub_verts', 'temp_verts')

        # the reference's optimizer (core/trainer.py:110-114: Adam, lr = SOLVER.BASE_LR 5e-5) runs inside the timed step: torch's fused
        # multi-tensor Adam -- not a path kernel, but a training number without the update would be incomplete.  Its in-place update bumps
        # the parameter versions, so the bf16 operand copies of the weights are re-cast every step, as in a real run.
        opt = torch.optim.Adam(params, lr=5e-5, fused=True)
        # ground truth of the auxiliary (IUV) supervision: synthetic DensePose tables of the real sizes (7829 vertices, 13774 faces; the licensed
        # UV_Processed.mat is not shipped) on the synthetic SMPL mesh, rendered on the device every step like the reference does with pytorch3d
        from whmr_amd.train.aux_supervision import aux_supervision_loss, render_iuv_targets
        from whmr_amd.utils.renderer import IUV_Renderer
        iuv_maker = IUV_Renderer(orig_size=(256, 256), output_size=(128, 128), dp=synth.make_densepose_tables(0, assets))
        gt_cam = torch.tensor([[0.9, 0.0, 0.0]], device=dev).expand(args.batch, -1).contiguous()

        class MeanSquares(torch.autograd.Function):
            """sum_t mean(t^2) over a list of tensors -- the synthetic stand-in for the reference's criteria -- in FOUR launches: one batched concatenation
            of the 27 supervised tensors into a flat vector, one square, one dot product with the constant per-element weights 1 / numel(t); the backward is
            one scaled copy whose pieces are views.  The same value and gradients as the per-tensor expression below (~190 launches: 27 x (pow, mean, add)
            and their backward nodes) and as round 5's _foreach_norm form (33 reduction launches, 0.25 ms on the stream the backward starts from)."""

            @staticmethod
            def forward(ctx, *ts):
                flat = torch.cat([t.detach().reshape(-1).float() for t in ts])
                w = _elem_weights(tuple(t.numel() for t in ts), flat.device)
                ctx.save_for_backward(flat, w)
                ctx.shapes = [t.shape for t in ts]
                return torch.dot(flat * flat, w)

            @staticmethod
            def backward(ctx, g):
                flat, w = ctx.saved_tensors
                gf = flat * w
                gf.mul_(2.0 * g)
                return tuple(p.view(sh) for p, sh in zip(torch.split(gf, [int(torch.Size(sh).numel()) for sh in ctx.shapes]), ctx.shapes))

        inv_cache = {}

        def _elem_weights(numels, device):                                             # built once (a constant of the output shapes)
            key = (numels, device)
            if key not in inv_cache:
                inv_cache[key] = torch.cat([torch.full((n,), 1.0 / n, dtype=torch.float32) for n in numels]).to(device)
            return inv_cache[key]

        def fwd_bwd():
            for p in params:
                p.grad = None
            out, _ = call(*a, is_train=True)
            sup = [out['smpl_out'][l][k] for l in range(1, 4) for k in keys]
            if args.loss == 'multi-tensor':
                loss = MeanSquares.apply(*sup)
            else:
                loss = sum(t.float().pow(2).mean() for t in sup)
            if out['dp_out']:
                # IUV head (AUX_SUPV_ON): the reference's dense-correspondence losses against ground truth RENDERED THIS STEP from the fitted mesh
                # (core/trainer.py:442-482) -- here the HIP rasteriser (whmr_amd.utils.renderer.IUV_Renderer) on the stage-3 mesh, detached
                # and the fused loss kernels (csrc/iuv_loss.hip) on the head's channels-last logits: same values as body_uv_losses on the target maps
                img, _ = render_iuv_targets(iuv_maker, out['smpl_out'][-1]['verts'].detach(), gt_cam, maps=False)
                loss = loss + aux_supervision_loss(out['dp_out'], None, iuv_image_gt=img)
            loss.backward()
            if red is not None:
                red.finish()
                if not sync_bn:
                    broadcast_buffers(m)                        # DDP broadcast_buffers: local BatchNorm running statistics follow rank 0 (identical on every rank under sync)
            return loss

        def train_step():
            loss = fwd_bwd()
            opt.step()
            return loss

        def train_step_serial():                 # the instrumented (per-launch event) step: no side stream, an event pair brackets its launch alone
            from whmr_amd.train import whmr_train as WT
            ov, WT.OVERLAP_HEAVY = WT.OVERLAP_HEAVY, False
            try:
                return train_step()
            finally:
                WT.OVERLAP_HEAVY = ov
        args.eager_step = train_step_serial
        args.dump_tree = lambda loss: {'loss': loss, 'grad': {n: p.grad for n, p in named}}
        if use_graph:
            from whmr_amd.train import capture_train_step
            with torch.enable_grad():
                replay, graph_loss = capture_train_step(m, fwd_bwd)       # forward + backward replayed; the optimizer step stays eager

            def graph_step():
                replay()
                opt.step()
                return graph_loss
            return graph_step, None, inp['x'], (256, 192)
        return train_step, None, inp['x'], (256, 192)
    raise SystemExit('unknown workload %s' % args.workload)


def cgroup_cpu_quota():
    """CPUs' worth of time the container's cgroup grants (cpu.max, v2; cfs quota, v1), or None when unlimited / unreadable: why 32 / 64 threads can be
    SLOWER than 16 on a 128-core host"""
    try:
        with open('/sys/fs/cgroup/cpu.max') as f:
            q, p = f.read().split()[:2]
        return None if q == 'max' else float(q) / float(p)
    except (OSError, ValueError):
        pass
    try:
        with open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us') as f:
            q = float(f.read())
        with open('/sys/fs/cgroup/cpu/cpu.cfs_period_us') as f:
            p = float(f.read())
        return None if q <= 0 else q / p
    except (OSError, ValueError):
        return None


def host_cpu_info():
    """CPU model string, physical cores, logical CPUs this process may run on ("core count and CPU model stated")"""
    model, cores = None, set()
    try:
        phys = core = None
        with open('/proc/cpuinfo') as f:
            for line in f:
                k, _, v = line.partition(':')
                k, v = k.strip(), v.strip()
                if k == 'model name' and model is None:
                    model = v
                elif k == 'physical id':
                    phys = v
                elif k == 'core id':
                    core = v
                elif not k and phys is not None:
                    cores.add((phys, core))
                    phys = core = None
            if phys is not None:
                cores.add((phys, core))
    except OSError:
        pass
    usable = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    return {'model': model, 'physical_cores': len(cores) or None, 'logical_cpus': os.cpu_count(), 'usable_cpus': usable, 'sched_affinity_cpus': usable,
            'cgroup_cpu_quota': cgroup_cpu_quota()}


def cpu_baseline(sd, x_cpu, size, heads=12):
    """Oracle (pure-PyTorch fp32 restatement of the reference ViT) on the host cores, bounded sample (~10-20 s).

    The box exposes 256 logical CPUs but the container's usable share is much smaller (more threads run slower), so a
    short sweep on 8 images picks the thread count, then the same batch-64 workload is timed at that setting.
    """
    from oracle.vit import vit_forward
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    best, sweep = None, {}
    with torch.no_grad():
        # one thread: the per-core figure (BASELINE.md 3 asks for it next to the all-core number); 2 crops, one warm pass
        torch.set_num_threads(1)
        vit_forward(sd, x_cpu[:1], num_heads=heads)
        t0 = time.perf_counter()
        vit_forward(sd, x_cpu[:2], num_heads=heads)
        one_thread = 2 / (time.perf_counter() - t0)
        for th in sorted({min(t, ncpu) for t in (8, 16, 32, 64)}):
            torch.set_num_threads(th)
            vit_forward(sd, x_cpu[:2], num_heads=heads)
            t0 = time.perf_counter()
            vit_forward(sd, x_cpu[:8], num_heads=heads)
            dt = time.perf_counter() - t0
            sweep[str(th)] = 8 / dt
            if best is None or dt < best[1]:
                best = (th, dt)
        torch.set_num_threads(best[0])
        n = x_cpu.shape[0]
        # The whole batch in ONE pass is not the host's best operating point: at 64 crops the fp32 activations (hidden 154 MB, attention scores
        # 118 MB) stream through DRAM, at 8 crops they stay in the last-level cache -- the short sweep above ran 8 crops and was 2.2x faster per image
        # than the batch-64 pass the round-4 line reported.  Both are timed now, the same 64 crops either way, and `value` is the
        # faster one; the outputs are the same numbers (images are independent), the parity leg takes the chunked pass's.
        t0 = time.perf_counter()
        vit_forward(sd, x_cpu, num_heads=heads)
        dt_one = time.perf_counter() - t0
        reps, t0 = 0, time.perf_counter()
        chunk = 8
        while reps < 1 or (time.perf_counter() - t0 < 8.0 and reps < 8):
            cpu_baseline.last_output = torch.cat([vit_forward(sd, x_cpu[i:i + chunk], num_heads=heads) for i in range(0, n, chunk)])
            reps += 1
        dt_chunks = (time.perf_counter() - t0) / reps
        dt = min(dt_one, dt_chunks)
    return {'value': n / dt, 'unit': 'images/sec', 'cores': best[0], 'kind': 'port',
            'cpu': host_cpu_info(), 'one_thread_images_per_sec': one_thread, 'thread_sweep_images_per_sec': sweep,
            'batch64_one_pass_images_per_sec': n / dt_one, 'batch64_in_chunks_of_8_images_per_sec': n / dt_chunks,
            'sample': 'oracle.vit.vit_forward fp32 (CPU restatement of the reference ViT) over one batch of %d %dx%d crops, torch threads = %d (best of a '
                      'short sweep on 8 crops: thread_sweep_images_per_sec; %d logical CPUs usable); value = the faster of ONE pass over the 64 crops '
                      '(%.1f s: activations stream through DRAM) and %d pass(es) in chunks of 8 crops (%.1f s each: cache-resident); '
                      'one_thread_images_per_sec: 2 crops on 1 thread' % (n, size[0], size[1], best[0], ncpu, dt_one, reps, dt_chunks)}


cpu_baseline.last_output = None


def parity_figures(out, ref):
    """(max-rel, element-wise) error of a device tensor against the CPU oracle's: max |a - b| / max |b|, and max over elements of
    |a - b| / (|b| + rms(b)) -- the metric the parity tests gate at 1e-4 (tests/conftest.py::ew_err)"""
    a, b = out.detach().double().cpu(), ref.detach().double().cpu()
    d = (a - b).abs()
    return {'max_rel': (d.max() / b.abs().max()).item(), 'elementwise': (d / (b.abs() + b.pow(2).mean().sqrt())).max().item()}


def time_steps(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def _named_tensors(obj, name, out):
    if torch.is_tensor(obj):
        out[name or 'output'] = obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _named_tensors(v, '%s.%s' % (name, k) if name else str(k), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _named_tensors(v, '%s.%d' % (name, i) if name else str(i), out)
    return out


def dump_outputs(tree, path, budget=60 << 20):
    """the tensors of ``tree`` (nested dicts / lists) as path/<dotted name>.npy: float64 and integer tensors as float64, the rest as float32.
    Within ``budget`` bytes of array data (60 MiB: the files' headers stay inside 64 MB): the smaller arrays whole, each larger one cut to an equal
    share of what is left, a sample of its flat elements at indices drawn from a generator seeded 0 (sorted) -- the same elements in every run
    of the same arguments."""
    import numpy as np
    arrays = {}
    for n, t in _named_tensors(tree, '', {}).items():
        exact64 = t.dtype == torch.float64 or not (t.is_floating_point() or t.dtype == torch.bool)
        arrays[n] = (t.detach().double() if exact64 else t.detach().float()).cpu()
    os.makedirs(path, exist_ok=True)
    left, files = budget, {}
    order = sorted(arrays, key=lambda n: arrays[n].numel() * arrays[n].element_size())
    for i, n in enumerate(order):
        a = arrays[n]
        keep = min(a.numel(), (left // (len(order) - i)) // a.element_size())
        if keep < a.numel():
            idx = torch.randperm(a.numel(), generator=torch.Generator().manual_seed(0))[:keep].sort().values
            a = a.reshape(-1)[idx]
        left -= a.numel() * a.element_size()
        np.save(os.path.join(path, n.replace(os.sep, '_') + '.npy'), a.numpy())
        files[n] = {'shape': list(arrays[n].shape), 'dtype': str(a.dtype).replace('torch.', ''), 'sampled': keep < arrays[n].numel()}
    return {'dir': path, 'bytes': budget - left, 'arrays': files}


def observed_clock(step, dev, n):
    """average shader clock (MHz) of one XCD while ``n`` steps run: a one-wave probe on a side stream reads s_memtime / s_memrealtime at its start and
    when the observed stream passes the end marker (whmr_clock_probe_*, csrc/ceilings.hip).  Outside every timed region."""
    from whmr_amd import _lib as L
    try:
        with L.ClockProbe(dev) as cp:
            for _ in range(n):
                step()
        return {'mhz': cp.mhz, 'window_ms': cp.seconds * 1e3, 'steps': n, 'probe_timed_out': cp.timed_out}
    except Exception as e:                      # noqa: BLE001   (an explanatory figure never costs the run its line)
        return {'error': '%s: %s' % (type(e).__name__, e)}


def secondary_rows(args, dev, x, budget_s=40.0):
    """Short legs behind the headline measurement of the DEFAULT run (put the parity-grade mode and BASELINE
    configs[2] / configs[3] under the driver's clock).  Each leg is a few steps of the same code path its own `--workload` / `--numerics`
    run times at length; legs are skipped (and say so) once the budget is spent.  Headline fields are untouched."""
    import copy
    from whmr_amd import _lib as L
    rows, t_start = {}, time.perf_counter()
    spent = lambda: time.perf_counter() - t_start
    ref = cpu_baseline.last_output

    # 3. BASELINE configs[3]: the training step at the per-GPU batch.  FIRST of the three: measured behind the other two legs (their HIP graphs, capture
    # pools and warm-up streams alive in the process) the same step takes 0.4 ms longer (19.80 vs 19.38 ms on one box; dedicated run 19.32-19.35); the other
    # two legs do not care about the order (4.28-4.31, 6.68-6.72)
    if spent() < budget_s:
        at = copy.copy(args)
        at.workload, at.numerics = 'whmr_train', 'bf16'
        with torch.enable_grad():
            stept, _, _, _ = build_workload(at, dev)
            ms = time_steps(stept, 20, 20)        # 0.4 s of warm-up: the package clock needs a few 100 ms to settle after the idle parity legs above
            clkt = observed_clock(stept, dev, 5)
        tf = VIT_FLOP_PER_IMG['whmr_train'] * args.batch / ms / 1e9
        rows['whmr_train'] = {'ms_per_step': ms, 'images_per_sec': args.batch / ms * 1e3, 'sclk_mhz_observed': clkt.get('mhz'),
                              'model_tflops': tf, 'frac': tf / 2500.0,
                              'roofline_note': 'whole-step figure: algorithmic forward + backward flops of ViT-B, the deconv pyramid, the Tz convolution and the IUV head '
                                               '(3 x forward, %.1f GF per image) / step time / the 2.5 PF dense bf16 peak -- everything else in the step (attention, '
                                               'LayerNorm / BatchNorm / GELU passes, the regressor loop, rasteriser, Adam) counts as time only' % (VIT_FLOP_PER_IMG['whmr_train'] / 1e9),
                              'workload': WORKLOAD['whmr_train']}
        del stept
    else:
        rows['whmr_train'] = {'skipped': 'secondary budget spent'}
    # 1. the headline workload in the bf16x3 numerics: parity-grade (1e-4 of the CPU reference) on the bf16 matrix pipes
    a3 = copy.copy(args)
    a3.numerics = 'bf16x3'
    with torch.no_grad():
        step3, _, _, _ = build_workload(a3, dev)
        ms = time_steps(step3, 16, 6)
        clk3 = observed_clock(step3, dev, 8)
        L.PROFILE = []
        out3 = step3()
        torch.cuda.synchronize()
        prof, L.PROFILE = L.PROFILE, None
    g = [(f, e0.elapsed_time(e1) * 1e-3) for (name, f, e0, e1) in prof if name == 'gemm_bf16x3']
    alg = sum(f for f, _ in g) / max(sum(t for _, t in g), 1e-12) / 1e12
    rows['vit224_bf16x3'] = {'ms_per_step': ms, 'images_per_sec': args.batch / ms * 1e3, 'sclk_mhz_observed': clk3.get('mhz'), 'gemm_algorithmic_TFLOPs': alg,
                             'mfma_issue_frac': 3.0 * alg / 2500.0,
                             'parity_vs_cpu_oracle': parity_figures(out3, ref) if ref is not None else None,
                             'note': 'same step, numerics bf16x3 (three bf16 MFMAs per product on hi/lo operand pairs, fp32 accumulate, erf GELU, fp32 '
                                     'LayerNorm / softmax): the mode that meets the 1e-4 tolerance AND runs on the bf16 matrix pipes; mfma_issue_frac = share of '
                                     'the 2.5 PF dense bf16 peak the pipes issue (3 x algorithmic); parity over the whole batch of %d crops' % args.batch}
    del step3, out3
    # 2. BASELINE configs[2]: full W-HMR forward (HIP graph), parity of the last stage vs the CPU oracle on the first 2 crops
    if spent() < budget_s:
        aw = copy.copy(args)
        aw.workload, aw.numerics = 'whmr', 'bf16'
        with torch.no_grad():
            stepw, _, _, _ = build_workload(aw, dev)
            ms = time_steps(stepw, 20, 10)
            clkw = observed_clock(stepw, dev, 10)
        tfw = VIT_FLOP_PER_IMG['whmr'] * args.batch / ms / 1e9
        rows['whmr'] = {'ms_per_step': ms, 'images_per_sec': args.batch / ms * 1e3, 'sclk_mhz_observed': clkw.get('mhz'), 'model_tflops': tfw, 'frac': tfw / 2500.0, 'cam_model_frames_per_step': 1,
                        'workload': WORKLOAD['whmr'] + '; ' + aw.full_x_note}
        try:                                # the north star's "achieved HBM GB/s on the sampler / LBS kernels", under the driver's clock
            with torch.no_grad():
                rows['whmr']['hbm_rows'] = whmr_hbm_rows(aw, dev)
            att = L.hbm_copy_ceiling(dev, mbytes=512, reps=3)
            for row in rows['whmr']['hbm_rows'].values():
                row['frac_of_attainable'] = row['achieved_GBps'] / att
            rows['whmr']['hbm_attainable_GBps'] = att
            rows['whmr']['hbm_rows_note'] = HBM_ROWS_NOTE
        except Exception as e:              # noqa: BLE001
            rows['whmr']['hbm_rows'] = {'error': '%s: %s' % (type(e).__name__, e)}
        if spent() < budget_s:
            rows['whmr']['parity_vs_cpu_oracle'] = whmr_parity(aw, dev, modes=('bf16', 'bf16x3'))
        del stepw
        aw.parity_ctx = None
    else:
        rows['whmr'] = {'skipped': 'secondary budget spent'}
    rows['seconds'] = spent()
    return rows


def whmr_parity(args, dev, modes=('bf16', 'bf16x3'), n_sample=2):
    """max-rel / element-wise error of theta, vertices and projected 2-D joints of the last regressor stage: the device forward of the WHOLE
    benchmark batch (first n_sample crops compared) against the CPU oracle, per numerics mode"""
    from oracle import whmr as OW
    from whmr_amd.models import whmr_net
    m, sd, assets, inp, kw = args.parity_ctx
    n_sample = min(n_sample, args.batch)
    cpu = {k: v[:n_sample].cpu() for k, v in inp.items()}
    full = kw['full_x'].cpu() if 'full_x' in kw else None
    if full is not None:
        full = full[:n_sample] if full.shape[0] > 1 else full.expand(n_sample, -1, -1, -1)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with torch.no_grad():
        ref_out, _ = OW.whmr_forward(sd, assets, cpu['x'], cpu['center'], cpu['scale'], cpu['bbox_height'], cpu['orig_shape'], cpu['bbox_info'], full_x=full,
                                     view='train')
    ref = ref_out['smpl_out'][-1]
    res = {}
    for mode in modes:
        mod = m if mode == m.numerics else whmr_net(None, assets=assets, numerics=mode)
        if mod is not m:
            mod.load_state_dict(sd, strict=True)
            mod = mod.to(dev).eval()
        with torch.no_grad():
            out, _ = mod(inp['x'], None, inp['center'], inp['scale'], inp['bbox_height'], inp['orig_shape'], inp['bbox_info'], view='train', **kw)
        o = out['smpl_out'][-1]
        res[mode] = {k: parity_figures(o[k][:n_sample], ref[k]) for k in ('theta', 'verts', 'kp_2d')}
    return res


def cpu_train_baseline(n_img=4):
    """CPU leg of the whmr_train workload: the oracle's training forward (oracle/train.py, the reference's arithmetic in plain PyTorch fp32)
    + torch autograd backward + Adam on a bounded sample of ``n_img`` 256x192 crops (the full batch of 64 would take minutes)."""
    from oracle import synth as osynth
    from oracle import train as OT
    threads = min(16, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    assets = osynth.make_assets(0)
    sd = osynth.make_state_dict(0, assets, with_cam_model=False)
    skip = ('running', 'cam_model', 'smpl', 'Dmap', 'points_grid', 'init_', 'num_batches', 'global_orient')
    p = {k: (v.clone().requires_grad_(True) if (v.is_floating_point() and not any(t in k for t in skip)) else v) for k, v in sd.items()}
    params = [v for v in p.values() if v.requires_grad]
    opt = torch.optim.Adam(params, lr=5e-5)
    inp = osynth.make_inputs(n_img, 7)
    keys = ('rotmat', 'pred_shape', 'pred_cam', 'kp_2d', 'kp_2d_w', 'kp_3d', 'verts', 'sub_verts', 'temp_verts')
    best = None
    for it in range(2):                                        # first pass warms the allocator / thread pool
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        dp = []
        outs = OT.whmr_forward_train(p, assets, inp['x'], inp['center'], inp['scale'], inp['bbox_height'], inp['orig_shape'], inp['bbox_info'],
                                     dp_out=dp)
        loss = sum(outs[l][k].pow(2).mean() for l in range(1, 4) for k in keys) + sum(v.pow(2).mean() for v in dp[0].values())
        loss.backward()
        opt.step()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return {'value': n_img / best, 'unit': 'images/sec', 'cores': threads, 'kind': 'port', 'cpu': host_cpu_info(),
            'sample': 'oracle.train.whmr_forward_train + autograd backward + Adam (CPU restatement of the reference training step, fp32), one '
                      'step on %d 256x192 crops (%.1f s), torch threads = %d' % (n_img, best, threads)}


def whmr_parity_and_fp32(args, dev, n_sample=2):
    """whmr workload extras: (1) max-rel error of theta / vertices / projected 2-D joints of the HIP forward against the CPU oracle on the
    first ``n_sample`` crops of the benchmark batch, in the benchmark numerics and in the fp32 parity mode; (2) ms per step of the fp32 mode."""
    from oracle import whmr as OW
    n_sample = min(n_sample, args.batch)
    m, sd, assets, inp, kw = args.parity_ctx
    cpu = {k: v[:n_sample].cpu() for k, v in inp.items()}
    full = kw['full_x'].cpu() if 'full_x' in kw else None
    if full is not None:                            # the oracle does not hoist: one frame per crop (the hoisted frame replicated)
        full = full[:n_sample] if full.shape[0] > 1 else full.expand(n_sample, -1, -1, -1)
    with torch.no_grad():
        ref_out, _ = OW.whmr_forward(sd, assets, cpu['x'], cpu['center'], cpu['scale'], cpu['bbox_height'], cpu['orig_shape'], cpu['bbox_info'], full_x=full,
                                     view='train')
    ref = ref_out['smpl_out'][-1]
    res = {}

    def rel(a, b):
        return ((a.double().cpu() - b.double()).abs().max() / b.double().abs().max()).item()
    from whmr_amd.models import whmr_net
    m32 = whmr_net(None, assets=assets, numerics='fp32')
    m32.load_state_dict(sd, strict=True)
    m32 = m32.to(dev).eval()
    # the device runs the WHOLE benchmark batch (the code path that was timed: e.g. the blocked-layout ViT kernels only engage from ~2k tokens);
    # the first n_sample crops of its output are compared -- every image is independent of the rest of the batch
    for tag, mod in ((args.numerics, m), ('fp32', m32)):
        with torch.no_grad():
            out, _ = mod(inp['x'], None, inp['center'], inp['scale'], inp['bbox_height'], inp['orig_shape'], inp['bbox_info'], view='train', **kw)
        o = out['smpl_out'][-1]
        res[tag] = {k: rel(o[k][:n_sample], ref[k]) for k in ('theta', 'verts', 'kp_2d')}
    a = (inp['x'], None, inp['center'], inp['scale'], inp['bbox_height'], inp['orig_shape'], inp['bbox_info'])
    with torch.no_grad():
        for _ in range(2):
            m32(*a, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            m32(*a, **kw)
        torch.cuda.synchronize()
    return res, (time.perf_counter() - t0) / 3 * 1e3


def whmr_hbm_rows(args, dev, n=20):
    """achieved HBM GB/s of the sampler launch and of one SMPL call: n back-to-back calls captured in a HIP graph (pure GPU time), inputs taken from a
    real forward of the benchmark batch; algorithmic bytes per SURVEY 8(d)"""
    m, sd, assets, inp, kw = args.parity_ctx
    B = inp['x'].shape[0]
    with torch.no_grad():
        out, _ = m(inp['x'], None, inp['center'], inp['scale'], inp['bbox_height'], inp['orig_shape'], inp['bbox_info'], view='train', **kw)
        last = out['smpl_out'][2]
        markers, cam = last['markers'].contiguous(), last['pred_cam'].contiguous()
        betas, rot = last['pred_shape'].contiguous(), last['rotmat'].reshape(B, 216).contiguous()
        ext, smpl = m.maf_extractor[2], m.regressor[2].smpl
        xc = torch.empty(B, m.regressor[2].fc1.in_features, dtype=torch.float32, device=dev)
        calls = {'maf_sample': (lambda: ext(markers, cam=cam, out=xc, want_point_feat=False),
                                B * markers.shape[1] * (4 * 256 * ext.im_feat.element_size() + 32 * 4.0)),
                 'smpl_call': (lambda: smpl.run(betas, rot, gram_schmidt=True, want_aa=True, want_smpl_joints=True, want_markers=True),
                               B * 84172.0 + 19.6e6)}
        rows = {}
        for name, (fn, byt) in calls.items():
            from whmr_amd._lib import side_stream
            side = side_stream(torch.cuda.current_device(), 2)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(n):
                    fn()
            g.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            sec = e0.elapsed_time(e1) * 1e-3 / n
            rows[name] = {'avg_us': sec * 1e6, 'algorithmic_bytes': byt, 'achieved_GBps': byt / sec / 1e9, 'frac_of_8TBps': byt / sec / 8e12}
    return rows


HBM_ROWS_NOTE = ('GPU time of ONE call, 20 calls replayed from a HIP graph on the tensors of a real forward (an eager call is host-launch bound and would '
                 'time the interpreter); maf_sample = one fused launch (projection + bilinear gather of 256 channels at 67 points + point MLP); smpl_call = '
                 'pose chain, pose-corrective blend + skinning, joint regression + stage tail (3 dependent launches); algorithmic bytes per SURVEY 8(d); both '
                 'are latency-bound at these sizes')


def cpu_whmr_baseline(args, n_img=4):
    """CPU leg of the whmr workload: the oracle's full forward (oracle/whmr.py, incl. the ResNet-50 of cam_model on one 600x800 frame) on a
    bounded sample of ``n_img`` crops"""
    from oracle import whmr as OW
    m, sd, assets, inp, kw = args.parity_ctx
    threads = min(16, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    cpu = {k: v[:n_img].cpu() for k, v in inp.items()}
    full = kw['full_x'][:1].cpu().expand(n_img, -1, -1, -1) if 'full_x' in kw else None     # the reference runs cam_model once per crop
    best = None
    with torch.no_grad():
        for _ in range(2):
            t0 = time.perf_counter()
            OW.whmr_forward(sd, assets, cpu['x'], cpu['center'], cpu['scale'], cpu['bbox_height'], cpu['orig_shape'], cpu['bbox_info'], full_x=full)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
    return {'value': n_img / best, 'unit': 'images/sec', 'cores': threads, 'kind': 'port', 'cpu': host_cpu_info(),
            'sample': 'oracle.whmr.whmr_forward fp32 (CPU restatement of WHMR.forward incl. cam_model on a 600x800 frame per crop, as the reference runs it), %d 256x192 crops (%.1f s), '
                      'torch threads = %d' % (n_img, best, threads)}


def gemm_source_digest():
    """sha256 over the GEMM kernel sources: profiles/*_gemm_traffic.json records the digest it was measured at"""
    import hashlib
    h = hashlib.sha256()
    for f in ('gemm_blk.hip', 'gemm_blk16_impl.h', 'gemm_blk_impl.h', 'gemm_blk_x3.hip', 'gemm_blk.h', 'gemm_bf16_big.hip', 'gemm_bf16_big_body.inc', 'gemm_bf16.hip', 'gemm_params.h', 'common.h'):
        with open(os.path.join(ROOT, 'w-hmr_amd', 'csrc', f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def gemm_traffic():
    """HBM bytes per GEMM launch from the committed rocprofv3 --pmc passes of this same command (profiles/), or None.  A file measured on
    other GEMM sources than the ones in the tree (digest mismatch) is STALE evidence and is not reported."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_vit224_gemm_traffic.json')), reverse=True):
        with open(path) as f:
            t = json.load(f)
        if t.get('gemm_source_digest') == gemm_source_digest():
            t['note'] = '%s: %s' % (os.path.basename(path), t['note'])
            return t
    return None


def reduce_max_time(dt, dist, dev):
    """max over ranks of the timed region (the slowest rank defines the step time)"""
    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    if dist is not None:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return t.item()


def aggregate_value(world, batch, steps, dt):
    """whole-job images/sec: every rank processes its own `batch` images per step (weak scaling, no collective)"""
    return world * batch * steps / dt


def shard_batch(global_batch, world, rank):
    """contiguous per-rank slice [lo, hi) of a global batch (partition = contiguous batch slices)"""
    per = global_batch // world
    return [rank * per, (rank + 1) * per]


def launch_ranks(args, argv):
    """`--gpus N` without a torch.distributed.run environment: start the N ranks as a CHILD process and relay rank 0's line.

    The parent never initialises HIP (no torch.cuda call before this point) and never exec()s: on this pool an exec from a process that
    has touched the GPU takes the machine down.  One rank per GPU, rendezvous on 127.0.0.1 (reference: train.py:26-33 spawns one process
    per GPU and calls init_process_group('nccl'))."""
    import socket
    import subprocess
    port = args.master_port
    if port is None:
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    import signal
    import threading
    # A hung rank (a collective that never completes, a wedged GPU) must not hang the driver: after
    # --rank-timeout the launcher ends the whole tree and exits 124.  torch elastic starts every worker in its OWN session
    # (SubprocessHandler: start_new_session=True), so killing the agent's process group reaches the agent only -- the ranks would survive as
    # orphans that keep the GPUs and the inherited stdout pipe.  Hence: snapshot the agent's descendants, SIGTERM the agent (its handler tears
    # its workers down), and after a grace period SIGKILL the agent and every descendant that is still alive.  The relay runs on a thread,
    # so a pipe that a surviving process keeps open cannot block the launcher either.
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env, start_new_session=True)
    found = []

    def relay():                                # the child's stderr goes straight through, its stdout is filtered for THE line
        try:
            for out in proc.stdout:
                if out.startswith('{') and '"metric"' in out:
                    found.append(out.strip())
                else:
                    sys.stdout.write(out)
        except ValueError:
            pass
    reader = threading.Thread(target=relay, daemon=True)
    reader.start()
    deadline = time.monotonic() + args.rank_timeout
    while proc.poll() is None and time.monotonic() < deadline:
        time.sleep(0.1)
    if proc.poll() is None:
        tree = process_tree(proc.pid)
        try:
            proc.send_signal(signal.SIGTERM)
        except ProcessLookupError:
            pass
        grace = time.monotonic() + min(10.0, max(2.0, 0.2 * args.rank_timeout))
        while time.monotonic() < grace and (proc.poll() is None or any(alive(q) for q in tree)):
            time.sleep(0.1)
        for q in set(tree) | set(process_tree(proc.pid)) | {proc.pid}:
            try:
                os.kill(q, signal.SIGKILL)
            except (ProcessLookupError, PermissionError):
                pass
        try:
            proc.wait(timeout=10)
        except subprocess.TimeoutExpired:
            pass
        # (the pipe is NOT closed from here: closing a file another thread is blocked reading can block in turn; once the tree is dead the relay
        #  thread sees EOF, and if some stranger still holds the write end the daemon thread simply dies with this process)
        reader.join(timeout=2)
        print('bench.py launcher: the %d ranks did not finish within %.0f s and were killed (agent + %d descendants)'
              % (args.gpus, args.rank_timeout, len(tree)), file=sys.stderr)
        return 124
    rc = proc.wait()
    reader.join(timeout=10)
    line = found[-1] if found else None
    if line is not None:
        print(line, flush=True)
    elif rc == 0:
        rc = 1
        print('bench.py launcher: the %d ranks exited 0 without printing a result line' % args.gpus, file=sys.stderr)
    return rc


def process_tree(pid):
    """pids of every descendant of ``pid`` (children of children ...), whatever session / process group they moved to"""
    try:
        import psutil
        return [c.pid for c in psutil.Process(pid).children(recursive=True)]
    except Exception:                           # noqa: BLE001   (psutil missing or the process already gone: walk /proc)
        kids = {}
        for d in os.listdir('/proc'):
            if d.isdigit():
                try:
                    with open('/proc/%s/stat' % d) as f:
                        ppid = int(f.read().rsplit(')', 1)[1].split()[1])
                    kids.setdefault(ppid, []).append(int(d))
                except (OSError, ValueError, IndexError):
                    pass
        out, todo = [], [pid]
        while todo:
            for c in kids.get(todo.pop(), []):
                out.append(c)
                todo.append(c)
        return out


def alive(pid):
    try:
        with open('/proc/%d/stat' % pid) as f:
            return f.read().rsplit(')', 1)[1].split()[0] != 'Z'
    except OSError:
        return False


def device_record(rank, local, dev, dry):
    """what this rank computes on -- `device_id` must be unique over the ranks of a run"""
    rec = {'rank': rank, 'local_rank': local, 'pid': os.getpid(), 'visible_devices': os.environ.get('HIP_VISIBLE_DEVICES', os.environ.get('ROCR_VISIBLE_DEVICES'))}
    if dry:
        rec.update(device='cpu', device_id='cpu:%d' % (0 if os.environ.get('WHMR_BENCH_DRYRUN_SAME_DEVICE') else rank))     # (test hook: a clashing map)
        return rec
    pr = torch.cuda.get_device_properties(dev)
    ident = None
    for attr in ('uuid', 'pci_bus_id'):                   # whichever this torch build exposes; the index alone cannot see a remapped visibility list
        v = getattr(pr, attr, None)
        if v is not None and str(v) not in ('', '0'):
            ident = '%s=%s' % (attr, v)
            break
    rec.update(device='cuda:%d' % dev.index, name=pr.name, arch=getattr(pr, 'gcnArchName', None), compute_units=pr.multi_processor_count,
               device_id='%s/%s/idx%d' % (rec['visible_devices'], ident, dev.index))
    return rec


def multi_rank_report(args, dist, world, dt_own, rank_map, red, dry, dev):
    """What explains an N > 1 number: every rank's own step time (a slow rank vs a slow exchange), the communicator's library
    version, the rank -> device map, and for the training step what the gradient exchange moved and how much of it finish() had to WAIT for."""
    own = {'ms_per_step': dt_own / args.steps * 1e3}
    # every rank's own step time as a plain float64 all_gather (the figure that must not get lost), the exchange details as objects
    tms = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
    dist.all_gather(tms, torch.tensor([own['ms_per_step']], dtype=torch.float64, device=dev))
    ms = [float(t.item()) for t in tms]
    rows = [None] * world
    if red is not None:
        waits = red.exposed_wait_ms()
        own.update(exposed_exchange_wait_ms_mean=sum(waits) / max(len(waits), 1), exposed_exchange_wait_ms_max=max(waits) if waits else 0.0,
                   collectives_per_step=getattr(args, 'reducer_stats', red.stats)['collectives'] / max(args.steps, 1),
                   bytes_exchanged_per_step=getattr(args, 'reducer_stats', red.stats)['bytes_exchanged'] / max(args.steps, 1),
                   buckets=len(red.buckets), bucket_bytes=[b['numel'] * 4 for b in red.buckets], unused_parameters=len(red.skipped))
    sg = getattr(args, 'sync_group', None)
    if sg is None and getattr(args, 'wrap', 'reducer') == 'ddp':
        from whmr_amd.parallel.sync_bn import auto_sync_groups      # torch nn.SyncBatchNorm modules: the group sync_of made for them
        sg = (auto_sync_groups() or [None])[0]
    if sg is not None:
        own.update(sync_bn_collectives_total=sg.collectives, sync_bn_bytes_total=sg.bytes)
    try:
        dist.all_gather_object(rows, own)
    except Exception as e:                       # noqa: BLE001
        rows = [dict(own, note='other ranks unavailable: %s' % type(e).__name__)]
    rep = {'per_rank_ms_per_step': {'min': min(ms), 'max': max(ms), 'all': ms},
           'ranks': rank_map,
           'backend': 'gloo (dryrun)' if dry else 'nccl = RCCL',
           'note': 'per_rank_ms_per_step: each rank\'s own time over the timed steps BEFORE the closing barrier (the line\'s ms_per_step is the max over ranks '
                   'incl. the barrier); launched with one process per GPU, fresh child of the launcher, rendezvous on 127.0.0.1'}
    if not dry:
        try:
            rep['rccl_version'] = '.'.join(str(v) for v in torch.cuda.nccl.version())
        except Exception as e:                           # noqa: BLE001
            rep['rccl_version'] = 'unavailable (%s)' % type(e).__name__
    if red is None and any('sync_bn_collectives_total' in r for r in rows if r):
        rep['sync_batchnorm'] = {'per_rank': [{k: r[k] for k in r if k.startswith('sync_bn_')} for r in rows if r],
                                 'note': 'wrap = ddp: torch DistributedDataParallel exchanges the gradients (its reducer keeps no counters here); the BatchNorm '
                                         'statistics of the nn.SyncBatchNorm modules travel as packed fp64 all-reduces of whmr_amd.parallel.sync_bn'}
    if red is not None:
        rep['gradient_exchange'] = {
            'per_rank': [{k: r[k] for k in r if k != 'ms_per_step'} for r in rows],
            'note': 'exposed_exchange_wait_ms = time inside GradReducer.finish() per step (event pair on the compute stream around the waits for the '
                    'exchange stream, straggler packs and the 1/world scaling): the part of the all-reduce the backward did not hide; bytes = fp32 '
                    'gradient bytes handed to all_reduce per step and rank (a ring moves 2 (N-1)/N of that over each link)'}
    return rep


def count_ranks(dist, dev):
    """the communicator's own rank count: all_reduce(SUM) of a one per rank (what `n_gpus` reports)"""
    if dist is None:
        return 1
    t = torch.ones(1, dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return int(round(t.item()))


def dryrun_workload(args, dev):
    """Stand-in step for `--dryrun-cpu` (tests): a tiny torch model on CPU.  For whmr_train it drives the REAL GradReducer / broadcast_buffers
    (incl. a parameter that never receives a gradient, as global_orient / cam_model in W-HMR) so the N > 1 bookkeeping of the entry point is
    covered by a gloo test.  Nothing here is the product path and its line is labelled "dryrun"."""
    torch.manual_seed(0)
    if os.environ.get('WHMR_BENCH_DRYRUN_HANG'):         # launcher test: ranks that are up (rendezvous done) and then never finish a step
        def hang():
            time.sleep(3600)
        return hang, None, torch.zeros(args.batch, 32), (1, 32)
    net = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.BatchNorm1d(64), torch.nn.GELU(), torch.nn.Linear(64, 8))
    unused = torch.nn.Linear(8, 8)               # registered with the reducer, never in the graph
    rank = int(os.environ.get('RANK', '0'))
    x = torch.randn(args.batch, 32, generator=torch.Generator().manual_seed(7 + rank))
    if args.workload != 'whmr_train':
        net.eval()
        return (lambda: net(x)), None, x, (1, 32)
    from whmr_amd.parallel import GradReducer, broadcast_buffers, convert_sync_batchnorm
    from whmr_amd.parallel.sync_bn import batch_norm_1d
    params = list(net.parameters()) + list(unused.parameters())
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if args.wrap == 'ddp':
        # the reference's wrap (core/trainer.py:83-86) around the stand-in: cross-rank BatchNorm statistics (this package's exchanges: batch_norm_1d ->
        # sync_of) under torch's OWN DistributedDataParallel reducer with find_unused_parameters -- pins the order of the BatchNorm all-reduces
        # relative to DDP's bucket all-reduces on ONE communicator across two gloo ranks
        from torch.nn.parallel import DistributedDataParallel

        class StandIn(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.net, self.unused = net, unused

            def forward(self, inp):
                h = batch_norm_1d(self.net[0](inp), self.net[1])
                return self.net[3](self.net[2](h))
        # (torch's DDP refuses a CPU module that holds nn.SyncBatchNorm layers -- "SyncBatchNorm layers only work with GPU modules" -- so the CPU stand-in
        # carries this package's mark on a plain BatchNorm1d, on the DEFAULT group: the same exchanges, sharing DDP's communicator; the two torch lines
        # verbatim run in tests/test_train_gpu.py::test_reference_syncbn_ddp_wrap_world1_rccl)
        mod = convert_sync_batchnorm(StandIn(), dedicated=False)
        ddp = DistributedDataParallel(mod, find_unused_parameters=True)
        opt = torch.optim.Adam(params, lr=1e-3)
        args.sync_bn, args.sync_group = True, mod.whmr_sync_group

        def step():
            opt.zero_grad(set_to_none=True)
            loss = ddp(x).pow(2).mean()
            loss.backward()
            opt.step()
            return loss
        args.dry_state = (net, unused, None)
        args.reducer = None
        return step, None, x, (1, 32)
    sync_bn = args.batchnorm == 'sync' or (args.batchnorm == 'auto' and world > 1)
    if sync_bn:                                  # the REAL cross-rank BatchNorm protocol (whmr_amd.parallel.sync_bn) on the stand-in's BatchNorm1d
        convert_sync_batchnorm(net)
    args.sync_bn, args.sync_group = sync_bn, getattr(net, 'whmr_sync_group', None)
    red = GradReducer(params, bucket_bytes=4096)
    opt = torch.optim.Adam(params, lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        h = batch_norm_1d(net[0](x), net[1])
        loss = net[3](net[2](h)).pow(2).mean()
        loss.backward()
        red.finish()
        if not sync_bn:
            broadcast_buffers(net)
        opt.step()
        return loss
    args.dry_state = (net, unused, red)
    args.reducer = red
    return step, None, x, (1, 32)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(launch_ranks(args, argv))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        raise SystemExit('bench.py: --gpus %d but WORLD_SIZE=%d' % (args.gpus, world))
    dry = args.dryrun_cpu
    if dry:
        dev = torch.device('cpu')
    else:
        if not torch.cuda.is_available():
            raise SystemExit('bench.py needs a HIP device: the hot path has no CPU fallback')
        torch.cuda.set_device(local)
        dev = torch.device('cuda', local)
    dist = None
    if world > 1 or ((args.always_bucket or args.wrap == 'ddp') and 'MASTER_ADDR' in os.environ and 'RANK' in os.environ):    # (one-rank RCCL smoke under torch.distributed.run)
        import torch.distributed as dist
        import datetime
        tmo = datetime.timedelta(seconds=max(60.0, min(args.rank_timeout, 1800.0)))      # a rank that never arrives fails the collective instead of hanging it
        if dry:
            dist.init_process_group('gloo', timeout=tmo)
        else:
            dist.init_process_group('nccl', device_id=dev, timeout=tmo)          # "nccl" IS RCCL on ROCm

    # who runs where: one record per rank, gathered over the communicator; two ranks on ONE device is a launch error (a wrong LOCAL_RANK /
    # HIP_VISIBLE_DEVICES map would "scale" by time-sharing a GPU), refused before anything is timed
    rank_map = [device_record(rank, local, dev, dry)]
    if dist is not None:
        # the clash test itself travels as one int64 per rank (a plain tensor all_gather: the collective every backend has); the readable records
        # follow as objects and are allowed to fail without costing the run its line
        import hashlib
        mine = int.from_bytes(hashlib.sha256(rank_map[0]['device_id'].encode()).digest()[:7], 'big')
        ids = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(ids, torch.tensor([mine], dtype=torch.int64, device=dev))
        ids = [int(t.item()) for t in ids]
        try:
            recs = [None] * world
            dist.all_gather_object(recs, rank_map[0])
            rank_map = recs
        except Exception as e:                   # noqa: BLE001
            rank_map = [dict(rank_map[0], note='records of the other ranks unavailable: %s: %s' % (type(e).__name__, e))]
        if len(set(ids)) != len(ids):
            raise SystemExit('bench.py: two ranks share a device: %s' % json.dumps(rank_map))

    def sync():
        if not dry:
            torch.cuda.synchronize()

    def barrier():
        sync()
        if dist is not None:
            dist.barrier()
        sync()

    if dry:
        step, sd, x, size = dryrun_workload(args, dev)
        L = None
    else:
        from whmr_amd import _lib as L
        step, sd, x, size = build_workload(args, dev)

    training = args.workload == 'whmr_train'
    prof = []
    with (torch.enable_grad() if training else torch.no_grad()):
        for _ in range(args.warmup):
            step()
        red = getattr(args, 'reducer', None)
        barrier()
        if red is not None:
            red.timing, red._wait_marks = True, []
            red.stats = {k: 0 for k in red.stats}
        t0 = time.perf_counter()
        for _ in range(args.steps - 1):
            step()
        last = step()
        sync()
        dt_own = time.perf_counter() - t0                # this rank's own time, before it waits for the others
        barrier()
        dt = time.perf_counter() - t0
        if red is not None:
            red.timing = False
            args.reducer_stats = dict(red.stats)     # snapshot: the instrumented step below also exchanges gradients
        dumped = None
        if args.dump_outputs and rank == 0:          # before the instrumented step below rewrites graph outputs and gradients
            dumped = dump_outputs(getattr(args, 'dump_tree', lambda out: out)(last), args.dump_outputs)
        del last
        if L is not None and args.full:
            # dominant-kernel timing: one instrumented step, HIP events around every GEMM launch on the launch stream
            L.PROFILE = []
            getattr(args, 'eager_step', step)()
            torch.cuda.synchronize()
            prof, L.PROFILE = L.PROFILE, None
            # shader clock while the timed workload runs (every rank runs the same steps: the training step has collectives), outside the timed region
            clock = {} if args.no_ceilings else observed_clock(step, dev, max(3, min(args.steps, 10)))
    dt = reduce_max_time(dt, dist, dev)
    n_ranks = count_ranks(dist, dev)
    multi = None
    if dist is not None:
        try:
            multi = multi_rank_report(args, dist, world, dt_own, rank_map, getattr(args, 'reducer', None), dry, dev)
        except Exception as e:                   # noqa: BLE001   (explanatory block only: never costs the run its line)
            multi = {'error': '%s: %s' % (type(e).__name__, e)}

    fp32_mode = args.numerics == 'fp32'                               # parity numerics: exact-f32 MFMA (v_mfma_f32_32x32x2_f32) GEMMs
    x3_mode = args.numerics == 'bf16x3'                               # parity-grade numerics on the bf16 pipes: three bf16 MFMAs per product
    gemm_name = 'gemm_f32' if fp32_mode else ('gemm_bf16x3' if x3_mode else 'gemm_bf16')
    gemm = [(f, e0.elapsed_time(e1) * 1e-3) for (name, f, e0, e1) in prof if name == gemm_name]
    traffic = gemm_traffic() if (args.full and args.workload == 'vit224' and not dry and args.numerics == 'bf16') else None    # the PMC passes measured the bf16 kernels
    n_launch = max(len(gemm), 1)
    flops_per_launch = sum(f for f, _ in gemm) / n_launch
    avg_s = sum(t for _, t in gemm) / n_launch
    achieved = flops_per_launch / avg_s / 1e12 if gemm else 0.0
    peak = 157.3 if fp32_mode else 2500.0                             # dense MFMA peak of the operand type, MI355X_MICROARCH.md (fp32 = the VALU rate)
    if rank == 0:
        value = aggregate_value(n_ranks, args.batch, args.steps, dt)
        if training:
            if getattr(args, 'sync_bn', False):
                bn = 'BatchNorm: SyncBatchNorm as in the reference (core/trainer.py:83) -- statistics / gradients of the 4 trained layers over all ranks, one packed fp64 all-reduce per layer and direction'
            else:
                bn = 'BatchNorm: local batch statistics + running-stat broadcast from rank 0 (--batchnorm local; the reference uses SyncBatchNorm, core/trainer.py:83)'
            par = 'dp%d (RCCL all-reduce of the gradients in 128 MiB buckets; %s)' % (n_ranks, bn)
            if args.wrap == 'ddp':
                par = 'dp%d (torch DistributedDataParallel(find_unused_parameters=True) over nn.SyncBatchNorm.convert_sync_batchnorm(model): the reference\'s own wrap, core/trainer.py:83-86)' % n_ranks
        else:
            par = 'replicas x%d (no data-path collective)' % n_ranks
        res = {
            'metric': METRIC.get(args.workload, args.workload) if not dry else 'dryrun (launcher / rank bookkeeping only)',
            'value': value,
            'unit': 'images/sec', 'n_gpus': n_ranks, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': dt / args.steps * 1e3, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
            'dtype': args.numerics, 'data': 'dryrun' if dry else 'synthetic',
            'config': {'workload': ('%s (%s), %dx%d crops, batch %d per GPU, random-init weights%s'
                                    % (WORKLOAD[args.workload], args.workload, size[0], size[1], args.batch,
                                       ('; ' + args.full_x_note + ('; eager module call, side streams folded into the main one' if args.serial else '; eager module call' if args.eager else '; replayed from one HIP graph'))
                                       if args.workload == 'whmr' else
                                       ('; synthetic L2 loss over the 27 supervised tensors as %s' % ('one concatenated weighted dot product (4 launches forward, 3 backward)' if args.loss == 'multi-tensor' else '27 x (pow, mean, add) expressions'))
                                       if args.workload == 'whmr_train' else '')) if not dry else 'dryrun-cpu stand-in',
                       'global_batch': n_ranks * args.batch, 'parallelism': par},
        }
        if args.ref_1gpu:
            res['efficiency_vs_1gpu'] = value / (n_ranks * args.ref_1gpu)
        if multi is not None:
            res['multi_gpu'] = multi
        if dumped is not None:
            res['dumped_outputs'] = dumped
        if not dry:
            res['model_tflops'] = VIT_FLOP_PER_IMG[args.workload] * n_ranks * args.batch * args.steps / dt / 1e12
        if not dry and args.full:
            res['roofline'] = {'bound': 'mfma', 'kernel': ('fp32 (exact-f32 MFMA) GEMM launches of one step (%d: gemm_f32_big_kernel for large M, the 64x64 / skinny kernels elsewhere)' % len(gemm)) if fp32_mode else
                               ('split-bf16 (bf16x3) GEMM launches of one step (%d: gemm_blk_kernel<X3>; achieved / frac count the ALGORITHMIC 2MNK flops -- the '
                                'matrix pipes issue three bf16 MFMAs per product, see mfma_issue_frac)' % len(gemm)) if x3_mode else
                               'bf16 MFMA GEMM launches of one step (%d: gemm_blk16_kernel on the blocked ViT path, gemm_tn_kernel for the weight gradients, gemm_bf16_big_kernel elsewhere)' % len(gemm),
                               'achieved': achieved, 'peak': peak, 'unit': 'TFLOP/s', 'frac': achieved / peak,
                               'flops_per_launch': flops_per_launch, 'avg_launch_us': avg_s * 1e6,
                               'traffic': traffic['bytes_per_launch'] if traffic else None,
                               'traffic_note': traffic['note'] if traffic else 'no PMC pass of the current GEMM sources committed'}
            # the launches of the step that are NOT GEMMs: attention on the matrix pipes + softmax VALU, the memory-bound passes;
            # `step_coverage` = instrumented launch time of one eager step / the timed step (the rest: launch gaps and un-instrumented small launches)
            other = {}
            for name, work, e0, e1 in prof:
                if name not in ('gemm_bf16', 'gemm_f32', 'gemm_bf16x3'):
                    o = other.setdefault(name, [0, 0.0, 0.0])
                    o[0] += 1; o[1] += work; o[2] += e0.elapsed_time(e1) * 1e-3
            rows = {}
            for name, (n, work, sec) in other.items():
                if name.endswith('_bytes'):
                    rows[name[:-6]] = {'bound': 'hbm', 'launches': n, 'avg_launch_us': sec / n * 1e6, 'algorithmic_bytes_per_launch': work / n,
                                       'achieved': work / sec / 1e9, 'peak': 8000.0, 'unit': 'GB/s', 'frac': work / sec / 8e12}
                else:
                    rows[name] = {'bound': 'mfma', 'launches': n, 'avg_launch_us': sec / n * 1e6, 'flops_per_launch': work / n,
                                  'achieved': work / sec / 1e12, 'peak': peak, 'unit': 'TFLOP/s', 'frac': work / sec / 1e12 / peak}
            if rows:
                res['roofline']['other_launches'] = rows
                res['roofline']['step_coverage'] = (sum(t for _, t in gemm) + sum(v[2] for v in other.values())) / (dt / args.steps)
                res['roofline']['step_coverage_note'] = ('instrumented launch time of ONE eager step (HIP events around every GEMM / attention / LayerNorm / gather launch) / the timed step; '
                                                         'the events add ~1 us per launch, so a step that is all instrumented launches reads slightly above 1')
            if x3_mode:
                res['roofline']['mfma_issue_frac'] = 3.0 * achieved / peak          # share of the dense bf16 MFMA peak the pipes actually issue
            # the box's own ceilings and clock, measured in THIS process after the timed region (datasheet numbers AND a measurement on the box):
            # `frac` (vs the nominal peak) stays the graded figure; `frac_of_attainable` prices the same launches against what the package sustains
            try:
                if args.no_ceilings:
                    raise RuntimeError('skipped (--no-ceilings)')
                mf = L.mfma_ceiling(dev)
                hbm = L.hbm_copy_ceiling(dev)
                issued = achieved * (3.0 if x3_mode else 1.0)
                res['roofline'].update(
                    attainable=None if fp32_mode else mf['tflops'], frac_of_attainable=None if fp32_mode else issued / mf['tflops'],
                    sclk_mhz_observed=clock.get('mhz'), sclk_probe=clock, attainable_sclk_mhz=mf['sclk_mhz'], hbm_attainable_GBps=hbm,
                    attainable_note='attainable = register-fed v_mfma_f32_16x16x32_bf16 stream on random operands, two waves per SIMD, %.2f s, no LDS / memory '
                                    '(whmr_mfma_ceiling) at the clock the governor grants it (attainable_sclk_mhz; the nominal peak assumes 2400 MHz); '
                                    'frac_of_attainable = MFMA flops ISSUED by the GEMM launches (3 x algorithmic in bf16x3) / attainable; sclk_mhz_observed = '
                                    's_memtime per s_memrealtime tick of one probe wave over %s steps of this workload; hbm_attainable_GBps = streaming copy of '
                                    '1 GiB (read + write bytes / time, whmr_hbm_copy)%s'
                                    % (mf['seconds'], clock.get('steps'), '; fp32 numerics: the bf16 ceiling does not apply to the f32 matrix instructions' if fp32_mode else ''))
            except Exception as e:                  # noqa: BLE001
                res['roofline']['attainable_error'] = '%s: %s' % (type(e).__name__, e)
            # (round 4 put a block of lab constants here -- `operand_read_ceiling` -- as if this run had measured them: removed.  What bounds `frac` is
            # measured by tools/gemm_stamps.py and tools/lab/dma_rate.hip; their outputs live under profiles/r05_gemm_stamps.txt,
            # profiles/r05_dma_rate_gemm_pattern.txt, with the budget in DESIGN 0.)
            if args.workload == 'whmr':
                res['cam_model_frames'] = {'gpu_per_step': {'hoisted': 1, 'per-crop': args.batch, 'none': 0}[args.full_x],
                                           'cpu_baseline_per_crop': 1,
                                           'note': 'machine-readable form of config.workload: the GPU step runs cam_model on this many 600x800 frames per '
                                                   'batch; the CPU leg replicates the frame per crop like demo/tester.py:161 (--full-x per-crop times the GPU that way)'}
                # the heavy chain behind the backbone, per launch, from the instrumented step (eager, side streams folded into the main one, one HIP-event pair
                # per launch: no concurrency and no profiler in these figures) -- deconv 1 / 2 / 3 and the composed Tz convolution's GEMM by their flop counts
                B_ = args.batch
                marks = {'deconv1': 2.0 * 4 * B_ * 16 * 12 * 256 * 4 * 768, 'deconv2': 2.0 * 4 * B_ * 32 * 24 * 256 * 4 * 256,
                         'deconv3': 2.0 * 4 * B_ * 64 * 48 * 256 * 4 * 256}
                marks['tz_composed_gemm'] = 2.0 * (B_ * 22 * 16) * 128 * 9216 * (4.0 / 3.0 if x3_mode else 1.0)      # (bf16x3: N = 256, K = 18432 -> 4x; / 3 below)
                hc = {}
                for name, f, e0, e1 in prof:
                    for k, fl in marks.items():
                        if name.startswith('gemm_bf16') and abs(f / ((3.0 if x3_mode else 1.0) * fl) - 1.0) < 1e-6:
                            us = e0.elapsed_time(e1) * 1e3
                            hc[k] = {'us': us, 'algorithmic_TFLOPs': fl / us / 1e6, 'frac': fl / us / 1e6 / peak}
                if hc:
                    res['heavy_chain'] = dict(hc, note='per-launch HIP-event times of the instrumented (serial, eager) step; frac = algorithmic 2MNK flops / time / the 2.5 PF '
                                                       'dense bf16 peak (bf16x3 issues three MFMAs per product)')
                # the HBM-bound rows of the north star: MAF sampler and SMPL (LBS) call
                res['hbm_rows'] = whmr_hbm_rows(args, dev)
                att = res['roofline'].get('hbm_attainable_GBps')
                if att:
                    for row in res['hbm_rows'].values():
                        row['frac_of_attainable'] = row['achieved_GBps'] / att
                res['hbm_rows_note'] = HBM_ROWS_NOTE
            if args.workload == 'whmr' and n_ranks == 1 and not args.no_parity:
                res['parity'], res['fp32_ms_per_step'] = whmr_parity_and_fp32(args, dev)
                res['parity_note'] = 'max-rel error of the last regressor stage (theta [B,85], vertices [B,6890,3], kp_2d [B,49,2]) of the full-batch device forward vs the CPU oracle on the ' \
                                     'first 2 crops of the batch; fp32_ms_per_step = the same step in the fp32 parity numerics (eager)'
            if not args.no_cpu and n_ranks == 1 and args.workload == 'whmr':
                res['cpu_baseline'] = cpu_whmr_baseline(args)
            elif not args.no_cpu and n_ranks == 1 and training:
                res['cpu_baseline'] = cpu_train_baseline()
            elif not args.no_cpu and n_ranks == 1 and sd is not None:
                res['cpu_baseline'] = cpu_baseline(sd, x.cpu(), size, 16 if args.workload == 'vitl256x192' else 12)
                try:
                    with torch.no_grad():
                        res['parity'] = dict(parity_figures(step(), cpu_baseline.last_output), numerics=args.numerics,
                                             note='backbone feature map [B, C, Hp, Wp] of the timed step vs the CPU oracle (oracle.vit.vit_forward, the '
                                                  'cpu_baseline leg) over the whole batch; the 1e-4 gate applies to the parity-grade numerics (fp32, bf16x3)')
                except Exception as e:                  # noqa: BLE001
                    res['parity'] = {'error': '%s: %s' % (type(e).__name__, e)}
            else:
                res['cpu_baseline'] = None
            if args.workload == 'vit224' and n_ranks == 1 and args.numerics == 'bf16' and not args.no_secondary:
                try:                                    # the secondary legs never cost the headline line: a failure is reported inside it
                    res['secondary'] = secondary_rows(args, dev, x)
                except Exception as e:                  # noqa: BLE001
                    import traceback
                    res['secondary'] = {'error': '%s: %s' % (type(e).__name__, e), 'where': traceback.format_exc().strip().splitlines()[-3:]}
        if dry:
            st = getattr(args, 'dry_state', None)
            if st is not None:
                net, unused, red = st
                res['dry'] = {'unused_grad_is_none': all(p.grad is None for p in unused.parameters()),
                              'grad_norm': float(sum(p.grad.pow(2).sum() for p in net.parameters()).sqrt()),
                              'running_mean_sum': float(net[1].running_mean.sum()), 'buckets': len(red.buckets) if red is not None else None,
                              'skipped_params': len(red.skipped) if red is not None else None, 'wrap': args.wrap,
                              'batchnorm_class': type(net[1]).__name__}
        print(json.dumps(res), flush=True)
    if dist is not None:
        # the workload's objects (DDP's reducer, GradReducer, their closures) hold the process group: released first, the group is freed by
        # destroy_process_group itself.  A gloo group still alive at interpreter exit aborts the rank now and then ("terminate called without
        # an active exception", signal 6)
        import gc
        del step, red
        for k in ('dry_state', 'reducer', 'sync_group', 'eager_step', 'parity_ctx', 'dump_tree'):
            args.__dict__.pop(k, None)
        gc.collect()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
