"""train.FusedAdam on the device (csrc/adam.hip): values against the float64 restatement (tests/adam_reference.py), the bf16 operand copies it
writes, skipped parameters, version bumps and the weight caches that hang on them, state_dict interchange with torch.optim.Adam(capturable=True),
and the step replayed from a HIP graph -- alone, and as the last node of a whole training iteration (capture_update_step)."""
import copy

import pytest
import torch

import adam_reference as AR
from conftest import ew_err

pytestmark = pytest.mark.gpu

# 1 .. 65: below / at / above a wave and the 4-wide vector body's ragged tail; 4097: a second workgroup holding one element; the matrices: N and K
# multiples of 64 or not, K % 4 != 0 (75, the 4-D weight viewed as [8, 75])
SHAPES = [(1,), (3,), (63,), (64,), (65,), (4097,), (96, 200), (130, 64), (8, 3, 5, 5)]
MATRICES = [(96, 200), (130, 64), (8, 3, 5, 5)]
LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8


def _data(shapes, steps, seed):
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(s, generator=g) for s in shapes]
    flats = [torch.randn(1 + sum(p.numel() for p in p0), generator=g) * (0.05 + 0.4 * k) for k in range(steps)]
    return p0, flats


def _views(flat, shapes, lead=1):
    """gradients as consecutive views of one flat buffer starting ``lead`` floats in (torch allocations are >= 256-byte aligned, so lead = 1 gives
    views 4 bytes off a 16-byte boundary, and the odd sizes in front move every later view to another residue): GradReducer's always_bucket layout"""
    out, off = [], lead
    for s in shapes:
        n = int(torch.Size(s).numel())
        out.append(flat[off:off + n].view(s))
        off += n
    return out


def _device_setup(dev, p0, shapes, numel_flat, aligned=False):
    params = [torch.nn.Parameter(p.to(dev)) for p in p0]
    if aligned:
        grads = [torch.zeros(s, device=dev) for s in shapes]
        flat = None
    else:
        flat = torch.zeros(numel_flat, device=dev)
        grads = _views(flat, shapes)
        assert all(g.data_ptr() % 4 == 0 for g in grads) and grads[0].data_ptr() % 16 == 4
    for p, g in zip(params, grads):
        p.grad = g
    return params, grads


def _fill(grads, flat_host, shapes, dev):
    for g, h in zip(grads, _views(flat_host, shapes)):
        g.copy_(h.to(dev))


@pytest.mark.parametrize('weight_decay', [0.0, 0.01])
def test_values_against_the_float64_restatement(dev, weight_decay):
    """4 steps over every shape, gradients 4-byte-aligned views of one flat buffer: p, exp_avg, exp_avg_sq against the float64 restatement fed the same
    fp32 gradients, ew_err <= 4 x the error of torch's own CPU fp32 Adam(foreach=False) on the same data (floor 2^-22).  The factor 4 allows for
    another order of the ~10 fp32 roundings of a step (FMA contraction)."""
    from whmr_amd.train import FusedAdam
    p0, flats = _data(SHAPES, 4, 100)
    params, grads = _device_setup(dev, p0, SHAPES, flats[0].numel())
    opt = FusedAdam(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=weight_decay)
    cpu = [torch.nn.Parameter(p.clone()) for p in p0]
    ref_opt = torch.optim.Adam(cpu, lr=LR, betas=BETAS, eps=EPS, weight_decay=weight_decay, foreach=False)
    for flat in flats:
        _fill(grads, flat, SHAPES, dev)
        opt.step()
        for p, g in zip(cpu, _views(flat, SHAPES)):
            p.grad = g.clone()
        ref_opt.step()
    torch.cuda.synchronize()
    rp, rm, rv, rt = AR.adam_run(p0, [_views(f, SHAPES) for f in flats], LR, BETAS, EPS, weight_decay)
    ours, theirs = {}, {}
    for i, (p, c) in enumerate(zip(params, cpu)):
        st, ct = opt.state[p], ref_opt.state[c]
        assert st['step'].item() == 4.0 and st['step'].dtype == torch.float32 and st['step'].dim() == 0 and st['step'].is_cuda
        for name, a, b, r in (('p', p.detach(), c.detach(), rp[i]), ('exp_avg', st['exp_avg'], ct['exp_avg'], rm[i]),
                              ('exp_avg_sq', st['exp_avg_sq'], ct['exp_avg_sq'], rv[i])):
            ours[name] = max(ours.get(name, 0.0), ew_err(a, r))
            theirs[name] = max(theirs.get(name, 0.0), ew_err(b, r))
        assert not torch.equal(p.detach().cpu(), p0[i])
    print('\nweight_decay %g: ew_err vs float64, FusedAdam %.3e, torch CPU fp32 Adam %.3e  (per tensor kind: %s)'
          % (weight_decay, max(ours.values()), max(theirs.values()), {k: '%.2e / %.2e' % (ours[k], theirs[k]) for k in ours}))
    for name in ours:
        assert ours[name] <= max(4 * theirs[name], 2.0 ** -22), (name, ours[name], theirs[name])


@pytest.mark.parametrize('aligned', [False, True], ids=['grads_4B_aligned', 'grads_16B_aligned'])
def test_tile_items_write_the_bf16_operand_copies(dev, aligned):
    """WeightOperands over the three matrices attached: after every step W == bf16(p) and W^T == W.t() bit for bit, the operands are marked current
    (refresh() has nothing to launch), and p / exp_avg / exp_avg_sq carry the same bits as the run without operands -- with gradients that force the
    dword path and with 16-byte aligned ones (the vector path where K % 4 == 0)."""
    from whmr_amd import _lib as L
    from whmr_amd.train import FusedAdam
    p0, flats = _data(MATRICES, 3, 200)
    params, grads = _device_setup(dev, p0, MATRICES, flats[0].numel(), aligned)
    plain, plain_grads = _device_setup(dev, p0, MATRICES, flats[0].numel(), aligned)
    wo = L.WeightOperands(params, {id(params[2]): (8, 75)})
    opt = FusedAdam(params, lr=LR, weight_decay=0.01)
    opt.attach_operands(wo)
    ref = FusedAdam(plain, lr=LR, weight_decay=0.01)
    assert opt.operands is wo and ref.operands is None
    for flat in flats:
        _fill(grads, flat, MATRICES, dev)
        _fill(plain_grads, flat, MATRICES, dev)
        opt.step()
        ref.step()
        assert wo.versions == [p._version for p in params]
        for p, q in zip(params, plain):
            w, wt = wo.copies[id(p)]
            assert torch.equal(w, p.detach().reshape(w.shape).bfloat16()), tuple(p.shape)
            assert torch.equal(wt, w.t()), tuple(p.shape)
            assert torch.equal(p.detach(), q.detach()), tuple(p.shape)
            for k in ('exp_avg', 'exp_avg_sq', 'step'):
                assert torch.equal(opt.state[p][k], ref.state[q][k]), (tuple(p.shape), k)
    assert not torch.equal(params[0].detach().cpu(), p0[0])
    # parameter storage replaced: the operands are stale, the optimizer goes back to flat items and leaves the copies to a new WeightOperands
    params[0].data = params[0].data.clone()
    assert wo.stale()
    opt.step()
    assert opt.operands is None
    ref.step()
    assert torch.equal(params[0].detach(), plain[0].detach())


def test_a_parameter_without_gradient_is_left_alone(dev):
    from whmr_amd.train import FusedAdam
    p0, flats = _data([(65,), (130, 64), (3,)], 2, 300)
    shapes = [tuple(p.shape) for p in p0]
    params, grads = _device_setup(dev, p0, shapes, flats[0].numel())
    opt = FusedAdam(params, lr=LR)
    _fill(grads, flats[0], shapes, dev)
    opt.step()
    before = [(p.detach().clone(), {k: v.clone() for k, v in opt.state[p].items()}, p._version) for p in params]
    params[1].grad = None
    _fill(grads, flats[1], shapes, dev)
    opt.step()
    torch.cuda.synchronize()
    for i, (p, (pb, sb, ver)) in enumerate(zip(params, before)):
        same = torch.equal(p.detach(), pb) and all(torch.equal(opt.state[p][k], sb[k]) for k in sb)
        if i == 1:
            assert same and opt.state[p]['step'].item() == 1.0 and p._version == ver
        else:
            assert not same and opt.state[p]['step'].item() == 2.0 and p._version > ver
    # all of it as the restatement has it
    rp, rm, rv, rt = AR.adam_run(p0, [_views(flats[0], shapes), [g if i != 1 else None for i, g in enumerate(_views(flats[1], shapes))]], LR)
    assert rt == [2, 1, 2]
    for p, r in zip(params, rp):
        assert ew_err(p.detach(), r) < 1e-6


def _small_vit(dev, sd, train=False):
    from whmr_amd.models.pose_vit import ViT
    m = ViT(img_size=(256, 192), embed_dim=128, depth=2, num_heads=2, qkv_bias=True, numerics='bf16')
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    return m.train() if train else m.eval()


def test_step_bumps_versions_and_the_weight_caches_follow(dev):
    """every updated parameter's _version grows; a bf16 ViT in eval mode (its bf16 weight copies are cached per version) answers differently after
    the step, and exactly as a fresh module loaded with the updated state_dict"""
    from oracle import synth
    from whmr_amd.train import FusedAdam
    m = _small_vit(dev, synth.make_vit_state(31, (256, 192), embed_dim=128, depth=2))
    x = synth.make_inputs(2, 32, (256, 192))['x'].to(dev)
    with torch.no_grad():
        y0 = m(x).clone()
    g = torch.Generator().manual_seed(33)
    for p in m.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    versions = [p._version for p in m.parameters()]
    opt = FusedAdam(m.parameters(), lr=1e-2)
    opt.step()
    assert all(p._version > v for p, v in zip(m.parameters(), versions))
    with torch.no_grad():
        y1 = m(x).clone()
        y2 = _small_vit(dev, {k: v.detach().cpu() for k, v in m.state_dict().items()})(x)
    assert not torch.equal(y0, y1)
    assert torch.equal(y1, y2)


def test_state_dict_interchanges_with_torch_adam_capturable(dev):
    """both directions: the loaded state carries the same bits, and one further step from it agrees with the source optimizer's further step.
    Bound of that step: two fp32 evaluations of the same formula from identical state differ by the roundings of one step on either side --
    p: its final rounding, 2 x 2^-24; exp_avg / exp_avg_sq: <= 4 roundings each side, 8 x 2^-24 = 2^-21 (ew_err)."""
    from whmr_amd.train import FusedAdam
    shapes = [(65,), (96, 200), (8, 3, 5, 5)]
    p0, flats = _data(shapes, 3, 400)
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=0.01)

    def make(cls, start, **extra):
        ps = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in start]
        return ps, cls(ps, **kw, **extra)

    def run(ps, opt, flat):
        for p, g in zip(ps, _views(flat, shapes)):
            p.grad = g.to(dev)
        opt.step()

    for src_cls, src_extra, dst_cls, dst_extra in ((FusedAdam, {}, torch.optim.Adam, dict(capturable=True)),
                                                   (torch.optim.Adam, dict(capturable=True), FusedAdam, {})):
        src_p, src = make(src_cls, p0, **src_extra)
        run(src_p, src, flats[0])
        run(src_p, src, flats[1])
        dst_p, dst = make(dst_cls, [p.detach() for p in src_p], **dst_extra)
        dst.load_state_dict(copy.deepcopy(src.state_dict()))
        for a, b in zip(src_p, dst_p):
            sa, sb = src.state[a], dst.state[b]
            assert sb['step'].dtype == torch.float32 and sb['step'].is_cuda and sb['step'].item() == 2.0
            for k in ('step', 'exp_avg', 'exp_avg_sq'):
                assert torch.equal(sa[k], sb[k]) and sa[k].data_ptr() != sb[k].data_ptr(), k
        assert dst.param_groups[0]['lr'] == LR and dst.param_groups[0]['capturable'] is True
        run(src_p, src, flats[2])
        run(dst_p, dst, flats[2])
        for a, b in zip(src_p, dst_p):
            assert src.state[a]['step'].item() == dst.state[b]['step'].item() == 3.0
            assert ew_err(b.detach(), a.detach()) <= 2.0 ** -21
            for k in ('exp_avg', 'exp_avg_sq'):
                assert ew_err(dst.state[b][k], src.state[a][k]) <= 2.0 ** -21, k


@pytest.mark.parametrize('step_as', ['host_tensor', 'python_number'])
def test_state_dict_of_a_default_torch_adam_loads_onto_the_device(dev, step_as):
    """what the reference checkpoints (trainer.py:362): a default torch.optim.Adam, capturable=False -- its ``step`` is a host tensor (a Python number
    in old files) and torch's load leaves it there; FusedAdam.load_state_dict moves it (the kernels dereference it), makes the group capturable
    again, and the next step agrees with torch's (bound: as in the interchange test above)"""
    from whmr_amd.train import FusedAdam
    shapes = [(65,), (96, 200)]
    p0, flats = _data(shapes, 3, 450)
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=0.01)
    src_p = [torch.nn.Parameter(p.clone().to(dev)) for p in p0]
    src = torch.optim.Adam(src_p, **kw)
    for flat in flats[:2]:
        for p, g in zip(src_p, _views(flat, shapes)):
            p.grad = g.to(dev)
        src.step()
    sd = copy.deepcopy(src.state_dict())
    assert sd['param_groups'][0]['capturable'] is False and not sd['state'][0]['step'].is_cuda
    if step_as == 'python_number':
        for st in sd['state'].values():
            st['step'] = int(st['step'].item())
    dst_p = [torch.nn.Parameter(p.detach().clone()) for p in src_p]
    dst = FusedAdam(dst_p, **kw)
    dst.load_state_dict(sd)
    assert dst.param_groups[0]['capturable'] is True
    for a, b in zip(src_p, dst_p):
        st = dst.state[b]
        assert st['step'].is_cuda and st['step'].dtype == torch.float32 and st['step'].dim() == 0 and st['step'].item() == 2.0
        for k in ('exp_avg', 'exp_avg_sq'):
            assert st[k].is_cuda and st[k].is_contiguous() and torch.equal(st[k], src.state[a][k])
    for ps, opt in ((src_p, src), (dst_p, dst)):
        for p, g in zip(ps, _views(flats[2], shapes)):
            p.grad = g.to(dev)
        opt.step()
    torch.cuda.synchronize()
    for a, b in zip(src_p, dst_p):
        assert dst.state[b]['step'].item() == 3.0
        assert ew_err(b.detach(), a.detach()) <= 2.0 ** -21
        for k in ('exp_avg', 'exp_avg_sq'):
            assert ew_err(dst.state[b][k], src.state[a][k]) <= 2.0 ** -21, k


def test_captured_optimizer_step_replays_like_eager_steps(dev):
    """the step alone in a HIP graph (static gradients, one stream): three replays with new gradients, the learning rate halved before the third
    through sync_hyperparameters(), leave p, exp_avg, exp_avg_sq and step with the bits of the same three eager steps from the same start"""
    from whmr_amd.train import FusedAdam
    p0, flats = _data(SHAPES, 4, 500)
    params, grads = _device_setup(dev, p0, SHAPES, flats[0].numel())
    eager, eager_grads = _device_setup(dev, p0, SHAPES, flats[0].numel())
    opt = FusedAdam(params, lr=LR, weight_decay=0.01)
    ref = FusedAdam(eager, lr=LR, weight_decay=0.01)
    # the common start: one eager step each (it creates the state and pushes the hyper-parameters, which a capture must not do)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _fill(grads, flats[0], SHAPES, dev)
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    _fill(eager_grads, flats[0], SHAPES, dev)
    ref.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for k in range(3):
        _fill(grads, flats[k + 1], SHAPES, dev)
        _fill(eager_grads, flats[k + 1], SHAPES, dev)
        if k == 2:
            for o in (opt, ref):
                o.param_groups[0]['lr'] *= 0.5
            opt.sync_hyperparameters()
        graph.replay()
        ref.step()
    torch.cuda.synchronize()
    for p, q in zip(params, eager):
        assert opt.state[p]['step'].item() == 4.0
        assert torch.equal(p.detach(), q.detach()), tuple(p.shape)
        for key in ('step', 'exp_avg', 'exp_avg_sq'):
            assert torch.equal(opt.state[p][key], ref.state[q][key]), (tuple(p.shape), key)
    # the halved rate was followed: the last step with the old rate ends elsewhere
    rp, _, _, _ = AR.adam_run(p0, [_views(f, SHAPES) for f in flats], LR, BETAS, EPS, 0.01, lrs=[LR, LR, LR, LR / 2])
    rq, _, _, _ = AR.adam_run(p0, [_views(f, SHAPES) for f in flats], LR, BETAS, EPS, 0.01)
    big = SHAPES.index((96, 200))
    assert ew_err(params[big].detach(), rp[big]) < 1e-6 < ew_err(params[big].detach(), rq[big])
    # an eager step right after the replays uploads its own table (a recorded upload is not an executed one) and a second capture of the same
    # optimizer finds a staging buffer ready: both continue the same trajectory
    _fill(grads, flats[1], SHAPES, dev)
    _fill(eager_grads, flats[1], SHAPES, dev)
    opt.reserve_staging()                                   # the first capture took the buffer the warm-up step had left
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        opt.step()
    opt.step()
    ref.step()
    opt.reserve_staging()
    graph3 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph3):
        opt.step()
    graph3.replay()
    ref.step()
    torch.cuda.synchronize()
    for p, q in zip(params, eager):
        assert opt.state[p]['step'].item() == 6.0 and torch.equal(p.detach(), q.detach()), tuple(p.shape)
    del graph2


def test_whole_training_step_with_the_update_replays_from_one_graph(dev, monkeypatch):
    """capture_update_step on a small bf16 ViT (256x192, embed 128, 2 heads, depth 2, batch 2): fn = zero_grad, forward, fixed-cotangent loss,
    backward, optimizer.step().  Before each of 3 replays the weights are snapshotted and the static input refilled; replay k's loss equals the
    loss of an eager training-mode forward of a fresh module holding that snapshot (bound of test_train_step_hip_graph_replay_matches_eager:
    1e-5 max(1, |loss|)) -- so the operand copies replay k - 1 wrote were the right ones -- the copies equal bf16(p) afterwards, no
    whmr_weights_prepare is in the graph, and the step count is warm-up + replays."""
    from oracle import synth
    from whmr_amd import _lib as L
    from whmr_amd.train import FusedAdam, capture_update_step
    m = _small_vit(dev, synth.make_vit_state(41, (256, 192), embed_dim=128, depth=2), train=True)
    x = synth.make_inputs(2, 42, (256, 192))['x'].to(dev)
    with torch.no_grad():
        shape = m.eval()(x).shape
    m.train()
    G = (torch.randn(shape, generator=torch.Generator().manual_seed(43)) / (shape[1] * shape[2] * shape[3]) ** 0.5).to(dev)
    opt = FusedAdam.for_model(m, lr=1e-3)
    wo = m._train_operands
    assert opt.operands is wo and len(wo.params) == 1 + 4 * 2

    def loss_of(model):
        return (model(x) * G).sum()

    def fn():
        opt.zero_grad()
        loss = loss_of(m)
        loss.backward()
        opt.step()
        return loss
    # refresh() launches whmr_weights_prepare exactly when it replaces ``versions``: none may happen from here on, in the warm-up or in the capture
    launches, refresh = [], L.WeightOperands.refresh

    def watched(self):
        before = self.versions
        out = refresh(self)
        if self is wo and self.versions is not before:
            launches.append(torch.cuda.is_current_stream_capturing())
        return out
    monkeypatch.setattr(L.WeightOperands, 'refresh', watched)
    warmup, replays = 2, 3
    replay, loss = capture_update_step(m, fn, opt, warmup=warmup)
    monkeypatch.undo()
    assert launches == [], launches
    assert opt.operands is wo and wo.versions == [p._version for p in wo.params]
    losses = []
    for k in range(replays):
        snapshot = {k_: v.detach().cpu().clone() for k_, v in m.state_dict().items()}
        x.copy_(synth.make_inputs(2, 50 + k, (256, 192))['x'].to(dev))
        versions = [p._version for p in m.parameters()]
        replay()
        torch.cuda.synchronize()
        assert all(p._version > v for p, v in zip(m.parameters(), versions))
        fresh = _small_vit(dev, snapshot, train=True)
        want = loss_of(fresh).item()
        losses.append(loss.item())
        print('replay %d: loss %.7f, eager forward of the snapshot %.7f' % (k, loss.item(), want))
        assert abs(loss.item() - want) < 1e-5 * max(1.0, abs(want)), (k, loss.item(), want)
        for p in wo.params:
            w, wt = wo.copies[id(p)]
            assert torch.equal(w, p.detach().reshape(w.shape).bfloat16()) and torch.equal(wt, w.t()), (k, tuple(p.shape))
    assert len(set(losses)) == replays
    for p in m.parameters():
        assert opt.state[p]['step'].item() == float(warmup + replays)
    # the forward of a replayed step found its operands current: refresh() launches nothing now either
    v = list(wo.versions)
    wo.refresh()
    assert wo.versions == v == [p._version for p in wo.params]
