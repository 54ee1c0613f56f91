"""FusedAdam's gradient guard on the device (csrc/adam.hip: whmr_adam_grad_sumsq, whmr_adam_guard_advance, whmr_adam_step_guarded): the global
norm against float64, a guarded step that does not clip against the unguarded one (bits), clipping against the float64 restatement
(tests/adam_guard_reference.py), skipped steps (nothing moves, the next step is step t + 1 of the applied ones), the guarded step replayed from a
HIP graph with the guard's row changed between replays, and the guard inside a whole captured training iteration.

One parameter set throughout: flat items of 1, 5, 4096 and 4097 elements (the last: two chunks, the second holding one element) and two tile items
with their bf16 W / W^T copies attached, 64 x 128 (whole tiles, K % 4 == 0: the 16-byte path when the pointers allow it) and 70 x 130 (ragged tiles,
dword path) -- with gradients that are 4-byte aligned views into one flat buffer, or 16-byte aligned tensors of their own."""
import math

import pytest
import torch

import adam_guard_reference as GR
from conftest import ew_err

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (5,), (4096,), (4097,), (64, 128), (70, 130)]
MATRICES = (4, 5)
NUMEL = sum(math.prod(s) for s in SHAPES)
LR, BETAS, EPS, WD = 1e-2, (0.9, 0.999), 1e-8, 0.01
ALIGNED = pytest.mark.parametrize('aligned', [False, True], ids=['grads_4B_aligned', 'grads_16B_aligned'])


def _views(flat, lead=1):
    """consecutive views of one flat buffer starting ``lead`` floats in: torch allocations are >= 256-byte aligned, so every view is 4 bytes off a
    16-byte boundary or more, and the odd sizes in front move later views to other residues (GradReducer's bucket layout)"""
    out, off = [], lead
    for s in SHAPES:
        n = math.prod(s)
        out.append(flat[off:off + n].view(s))
        off += n
    return out


_G = torch.Generator().manual_seed(700)
P0 = [torch.randn(s, generator=_G) for s in SHAPES]
FLATS = [torch.randn(1 + NUMEL, generator=_G) * (0.05 + 0.4 * k) for k in range(4)]          # host gradients of four steps, never modified
NORMS = [GR.global_norm(_views(f)) for f in FLATS]


class _Rig:
    """parameters on the device with static gradient tensors, WeightOperands over the two matrices, and a FusedAdam over all of it"""

    def __init__(self, dev, aligned, **kw):
        from whmr_amd import _lib as L
        from whmr_amd.train import FusedAdam
        self.dev = dev
        self.params = [torch.nn.Parameter(p.to(dev)) for p in P0]
        if aligned:
            self.grads = [torch.zeros(s, device=dev) for s in SHAPES]
            assert all(g.data_ptr() % 16 == 0 for g in self.grads)
        else:
            self.flat = torch.zeros(1 + NUMEL, device=dev)
            self.grads = _views(self.flat)
            assert all(g.data_ptr() % 4 == 0 for g in self.grads) and self.grads[0].data_ptr() % 16 == 4
        for p, g in zip(self.params, self.grads):
            p.grad = g
        self.wo = L.WeightOperands([self.params[i] for i in MATRICES])
        self.opt = FusedAdam(self.params, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, **kw)
        self.opt.attach_operands(self.wo)

    def fill(self, host_views):
        for g, h in zip(self.grads, host_views):
            g.copy_(h.to(self.dev))

    def step(self, host_views):
        self.fill(host_views)
        self.opt.step()

    def snapshot(self):
        """every tensor a step may write, cloned: p, exp_avg, exp_avg_sq, step per parameter and both bf16 copies per matrix"""
        out = []
        for p in self.params:
            st = self.opt.state[p]
            out += [p.detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone(), st['step'].clone()]
        for i in MATRICES:
            out += [c.clone() for c in self.wo.copies[id(self.params[i])]]
        return out


def _same_bits(a, b):
    # NaN-proof: compare the bit patterns
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape
               and torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8)) for x, y in zip(a, b))


def _bad(kind):
    """FLATS[1]'s gradients with one non-finite element: the single element of the 4097 item's second chunk, or the last row and column of the
    70 x 130 item (its ragged corner tile)"""
    views = [v.clone() for v in _views(FLATS[1])]
    if kind == 'nan_last_of_4097':
        views[3][-1] = float('nan')
    else:
        views[5][-1, -1] = float('inf')
    return views


@ALIGNED
def test_grad_norm_against_float64_and_run_to_run(dev, aligned):
    """opt.grad_norm against the float64 norm of the same gradients: relative error <= 1e-6.  Derivation: a thread squares and adds <= 16 elements
    in fp32, <= 16 x 2^-24 < 1.0e-6 relative on its sum of non-negative terms; everything across threads is in double; the square root halves it
    and the result is rounded to fp32 once (6e-8): <= ~5.6e-7, a 2 x margin.  A second optimizer on the same inputs gives the same bits."""
    got = []
    for _ in range(2):
        rig = _Rig(dev, aligned, skip_nonfinite=True)
        for k in range(2):
            rig.step(_views(FLATS[k]))
            got.append(rig.opt.grad_norm.clone())
            rel = abs(got[-1].item() - NORMS[k]) / NORMS[k]
            print('\nstep %d: grad_norm %.9g, float64 %.12g, relative error %.3e' % (k, got[-1].item(), NORMS[k], rel))
            assert got[-1].dtype == torch.float32 and got[-1].dim() == 0 and got[-1].is_cuda
            assert rel <= 1e-6, (k, got[-1].item(), NORMS[k])
        assert rig.opt.guard_summary() == dict(grad_norm=got[-1].item(), clip_coef=1.0, applied=True, steps_seen=2, steps_skipped=0)
    assert _same_bits(got[:2], got[2:])


@ALIGNED
def test_a_guarded_step_that_does_not_clip_has_the_unguarded_bits(dev, aligned):
    """max_grad_norm = 1e30: three guarded steps and three unguarded ones from the same start leave p, exp_avg, exp_avg_sq, step and both bf16 copies
    bit-identical, and clip_coef is exactly 1"""
    guarded, plain = _Rig(dev, aligned, max_grad_norm=1e30), _Rig(dev, aligned)
    assert plain.opt._guard_state is None
    for k in range(3):
        guarded.step(_views(FLATS[k]))
        plain.step(_views(FLATS[k]))
        assert guarded.opt.clip_coef.item() == 1.0
        assert _same_bits(guarded.snapshot(), plain.snapshot()), k
    assert plain.opt._guard_state is None and plain.opt._partials is None and plain.opt._guard_cfg is None          # guard off allocates nothing
    assert not torch.equal(guarded.params[5].detach().cpu(), P0[5])
    assert guarded.opt.state[guarded.params[0]]['step'].item() == 3.0


@ALIGNED
def test_clipped_steps_against_the_float64_restatement(dev, aligned):
    """max_grad_norm = 0.25 x the float64 norm of step 1, three steps (all clip: the later gradients are larger).  p / exp_avg / exp_avg_sq against
    the float64 restatement fed the same fp32 gradients: ew_err <= 4 x the error of torch's own CPU fp32 clip_grad_norm_ + Adam(foreach=False) on
    the same data, floor 2^-22 (the bound of test_adam_gpu.py::test_values_against_the_float64_restatement).  clip_coef against the restatement:
    <= 2e-6 relative (the norm's 1e-6 plus one division and one rounding to fp32).  The bf16 copies equal bf16(p); p.grad is not rewritten."""
    max_norm = 0.25 * NORMS[0]
    rig = _Rig(dev, aligned, max_grad_norm=max_norm)
    cpu = [torch.nn.Parameter(p.clone()) for p in P0]
    ref_opt = torch.optim.Adam(cpu, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, foreach=False)
    rp, rm, rv, rt, log = GR.guarded_run(P0, [_views(f) for f in FLATS[:3]], LR, BETAS, EPS, WD, max_grad_norm=max_norm)
    for k in range(3):
        rig.step(_views(FLATS[k]))
        coef = rig.opt.clip_coef.item()
        rel = abs(coef - log[k]['coef']) / log[k]['coef']
        print('\nstep %d: clip_coef %.9g, restatement %.12g, relative error %.3e' % (k, coef, log[k]['coef'], rel))
        assert log[k]['coef'] < 1.0 and rel <= 2e-6
        assert all(torch.equal(g.cpu(), h) for g, h in zip(rig.grads, _views(FLATS[k])))
        for p, g in zip(cpu, _views(FLATS[k])):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(cpu, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=False)
        ref_opt.step()
    ours, theirs = {}, {}
    for i, (p, c) in enumerate(zip(rig.params, cpu)):
        st, ct = rig.opt.state[p], ref_opt.state[c]
        assert st['step'].item() == 3.0
        for name, a, b, r in (('p', p.detach(), c.detach(), rp[i]), ('exp_avg', st['exp_avg'], ct['exp_avg'], rm[i]),
                              ('exp_avg_sq', st['exp_avg_sq'], ct['exp_avg_sq'], rv[i])):
            ours[name] = max(ours.get(name, 0.0), ew_err(a, r))
            theirs[name] = max(theirs.get(name, 0.0), ew_err(b, r))
    print('ew_err vs float64, guarded FusedAdam / torch CPU fp32 clip_grad_norm_ + Adam: %s' % {k: '%.2e / %.2e' % (ours[k], theirs[k]) for k in ours})
    for name in ours:
        assert ours[name] <= max(4 * theirs[name], 2.0 ** -22), (name, ours[name], theirs[name])
    for i in MATRICES:
        w, wt = rig.wo.copies[id(rig.params[i])]
        assert torch.equal(w, rig.params[i].detach().bfloat16()) and torch.equal(wt, w.t())


@ALIGNED
@pytest.mark.parametrize('kind', ['nan_last_of_4097', 'inf_last_of_70x130'])
def test_a_non_finite_step_is_skipped_whole(dev, aligned, kind):
    """good, bad, good with skip_nonfinite: after the bad step every p / exp_avg / exp_avg_sq / step and both copies carry the bits they had before
    it, steps_skipped == 1, steps_seen == 2, apply == 0; after the following good step everything carries the bits of a second optimizer that
    only ever saw the two good steps"""
    rig, twin = _Rig(dev, aligned, skip_nonfinite=True), _Rig(dev, aligned, skip_nonfinite=True)
    rig.step(_views(FLATS[0]))
    before = rig.snapshot()
    rig.step(_bad(kind))
    assert not math.isfinite(rig.opt.grad_norm.item())
    assert _same_bits(rig.snapshot(), before)
    s = rig.opt.guard_summary()
    assert (s['steps_skipped'], s['steps_seen'], s['applied'], s['clip_coef']) == (1, 2, False, 0.0), s
    assert rig.opt.steps_skipped.item() == 1 and rig.opt.steps_seen.item() == 2 and rig.opt.steps_skipped.dtype == torch.int64
    rig.step(_views(FLATS[2]))
    twin.step(_views(FLATS[0]))
    twin.step(_views(FLATS[2]))
    assert _same_bits(rig.snapshot(), twin.snapshot())
    assert rig.opt.state[rig.params[0]]['step'].item() == 2.0 and not _same_bits(rig.snapshot(), before)
    s = rig.opt.guard_summary()
    assert (s['steps_skipped'], s['steps_seen'], s['applied'], s['clip_coef']) == (1, 3, True, 1.0), s
    assert abs(s['grad_norm'] - NORMS[2]) <= 1e-6 * NORMS[2]


@pytest.mark.parametrize('kind', ['nan_last_of_4097', 'inf_last_of_70x130'])
def test_without_the_guard_a_non_finite_gradient_reaches_the_weights(dev, kind):
    """skip_nonfinite=False and no clipping is today's optimizer: the bad element's parameter becomes NaN, nothing of the guard exists"""
    rig = _Rig(dev, False)
    rig.step(_views(FLATS[0]))
    rig.step(_bad(kind))
    i = 3 if kind == 'nan_last_of_4097' else 5
    assert torch.isnan(rig.params[i].detach().reshape(-1)[-1]).item()
    assert torch.isfinite(rig.params[2].detach()).all().item()
    assert rig.opt._guard_state is None
    # ... and clipping without skip_nonfinite propagates it as torch's clip_grad_norm_ does: the NaN norm makes every coefficient NaN
    if kind == 'nan_last_of_4097':
        clip = _Rig(dev, False, max_grad_norm=1.0)
        clip.step(_bad(kind))
        assert math.isnan(clip.opt.clip_coef.item()) and clip.opt.guard_summary()['applied'] is True
        assert all(torch.isnan(p.detach()).all().item() for p in clip.params)


def test_captured_guarded_step_replays_like_eager_steps(dev, monkeypatch):
    """one eager guarded step, then one guarded step() captured over the static gradient buffers and replayed with good, NaN, good, clipped (x 40)
    and -- after set_grad_guard(max_grad_norm=...) + sync_hyperparameters() -- good gradients again, now clipped: states, copies, norm,
    coefficient and counters carry the bits of the same sequence stepped eagerly on a twin.  The guard cannot be changed, nor its buffers
    created, inside a capture."""
    from whmr_amd.train import FusedAdam
    max_norm = 2.0 * max(NORMS)
    rig, twin = _Rig(dev, False, max_grad_norm=max_norm, skip_nonfinite=True), _Rig(dev, False, max_grad_norm=max_norm, skip_nonfinite=True)
    from whmr_amd import _lib as L
    side = L.side_stream(dev, 2)                                           # the package's warm-up stream (capture_update_step's): no new stream
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rig.step(_views(FLATS[0]))
    torch.cuda.current_stream().wait_stream(side)
    twin.step(_views(FLATS[0]))
    torch.cuda.synchronize()
    state_ptr = rig.opt.grad_norm.data_ptr()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rig.opt.step()
    sequence = [_views(FLATS[1]), _bad('nan_last_of_4097'), _views(FLATS[2]), [40.0 * v for v in _views(FLATS[3])], _views(FLATS[1])]
    coefs = []
    for k, views in enumerate(sequence):
        if k == 4:
            for r in (rig, twin):
                r.opt.set_grad_guard(max_grad_norm=0.5 * NORMS[1])
            rig.opt.sync_hyperparameters()
        rig.fill(views)
        graph.replay()
        rig.opt.mark_updated()
        twin.step(views)
        coefs.append(rig.opt.clip_coef.item())
        assert _same_bits(rig.snapshot(), twin.snapshot()), k
        assert _same_bits([rig.opt._guard_state], [twin.opt._guard_state]), (k, rig.opt.guard_summary(), twin.opt.guard_summary())
    assert rig.opt.grad_norm.data_ptr() == state_ptr                      # replays write the buffer the views were taken from
    print('\nclip_coef per replay: %s' % coefs)
    assert coefs[0] == 1.0 and coefs[1] == 0.0 and coefs[2] == 1.0 and 0.0 < coefs[3] < 0.1
    assert abs(coefs[4] - 0.5) <= 2e-6 * 0.5                               # replay 0 had the same gradients and did not clip: the new row was followed
    s = rig.opt.guard_summary()
    assert (s['steps_seen'], s['steps_skipped'], s['applied']) == (6, 1, True), s
    assert rig.opt.state[rig.params[0]]['step'].item() == 5.0
    # inside a capture (the stream is only SAID to be capturing here: these raise before anything is launched or recorded)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    rig.opt.set_grad_guard(max_grad_norm=1.0)
    with pytest.raises(RuntimeError, match='changed inside a graph capture'):
        rig.opt.step()
    with pytest.raises(RuntimeError, match='changed inside a graph capture'):
        rig.opt.sync_hyperparameters()
    rig.opt.set_grad_guard(max_grad_norm=0.5 * NORMS[1])
    monkeypatch.undo()
    late = _Rig(dev, False)
    late.step(_views(FLATS[0]))                                            # an unguarded warm-up step: state exists, the guard's buffers do not
    late.opt.set_grad_guard(skip_nonfinite=True)
    late.opt.sync_hyperparameters()
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='run a warm-up step'):
        late.opt.step()
    monkeypatch.undo()
    late.step(_views(FLATS[1]))
    assert late.opt.steps_seen.item() == 1 and isinstance(late.opt, FusedAdam)


def _small_vit(dev, sd):
    from whmr_amd.models.pose_vit import ViT
    m = ViT(img_size=(256, 192), embed_dim=128, depth=2, num_heads=2, qkv_bias=True, numerics='bf16')
    m.load_state_dict(sd, strict=True)
    return m.to(dev).train()


def test_guard_inside_a_whole_captured_training_step(dev):
    """capture_update_step on the small bf16 ViT of test_adam_gpu.py (256x192, embed 128, 2 heads, depth 2, batch 2) with
    FusedAdam.for_model(model, max_grad_norm=1.0, skip_nonfinite=True): after each of two replays the loss is finite, opt.grad_norm equals the
    float64 norm of the .grad tensors the replay left within 1e-6 relative (bound: as in test_grad_norm_against_float64_and_run_to_run), nothing
    was skipped, and the coefficient is the one that norm implies"""
    from oracle import synth
    from whmr_amd.train import FusedAdam, capture_update_step
    m = _small_vit(dev, synth.make_vit_state(41, (256, 192), embed_dim=128, depth=2))
    x = synth.make_inputs(2, 42, (256, 192))['x'].to(dev)
    with torch.no_grad():
        shape = m.eval()(x).shape
    m.train()
    G = torch.randn(shape, generator=torch.Generator().manual_seed(43)).to(dev)
    opt = FusedAdam.for_model(m, lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    assert opt.operands is m._train_operands and opt.max_grad_norm == 1.0 and opt.skip_nonfinite

    def fn():
        opt.zero_grad()
        loss = (m(x) * G).sum()
        loss.backward()
        opt.step()
        return loss
    replay, loss = capture_update_step(m, fn, opt, warmup=1)
    for k in range(2):
        x.copy_(synth.make_inputs(2, 50 + k, (256, 192))['x'].to(dev))
        replay()
        torch.cuda.synchronize()
        want = GR.global_norm([p.grad.detach().cpu() for p in m.parameters() if p.grad is not None])
        got, coef = opt.grad_norm.item(), opt.clip_coef.item()
        print('\nreplay %d: loss %.6f, grad_norm %.9g, float64 %.12g (relative error %.3e), clip_coef %.6g'
              % (k, loss.item(), got, want, abs(got - want) / want, coef))
        assert math.isfinite(loss.item())
        assert abs(got - want) <= 1e-6 * want
        assert abs(coef - GR.clip_coef(want, 1.0)) <= 2e-6 * GR.clip_coef(want, 1.0)
    s = opt.guard_summary()
    assert s['steps_skipped'] == 0 and s['steps_seen'] == 3 and s['applied'] is True
    for p in m.parameters():
        if p.grad is not None:
            assert opt.state[p]['step'].item() == 3.0
