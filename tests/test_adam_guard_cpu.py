"""Host side of FusedAdam's gradient guard: the float64 restatement (tests/adam_guard_reference.py) is torch's clip_grad_norm_ + Adam, the three
entry points have their wrappers, and the options are validated and stay out of param_groups."""
import math

import pytest
import torch

import adam_guard_reference as GR
from conftest import ew_err

SHAPES = [(1,), (65,), (96, 200), (8, 3, 5, 5)]


@pytest.mark.parametrize('case,max_norm_factor,weight_decay', [('coef_below_1', 0.25, 0.0), ('coef_is_1', 1e6, 0.0), ('weight_decay', 0.25, 0.01)])
def test_guard_restatement_is_torch_clip_grad_norm_and_adam(case, max_norm_factor, weight_decay):
    """float64 CPU parameters, 4 steps of clip_grad_norm_(max_norm) + torch.optim.Adam: p, exp_avg, exp_avg_sq agree with the restatement to 1e-12
    (tests/test_adam_cpu.py's bound for restatement against torch), and so do the norm and the coefficient torch reports / implies"""
    g = torch.Generator().manual_seed(21)
    p0 = [torch.randn(s, generator=g, dtype=torch.float64) for s in SHAPES]
    grads = [[torch.randn(s, generator=g, dtype=torch.float64) * (0.1 + k) for s in SHAPES] for k in range(4)]
    max_norm = max_norm_factor * GR.global_norm(grads[0])
    params = [torch.nn.Parameter(x.clone()) for x in p0]
    opt = torch.optim.Adam(params, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    norms = []
    for gs in grads:
        for p, gr in zip(params, gs):
            p.grad = gr.clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0, error_if_nonfinite=False)))
        opt.step()
    rp, rm, rv, rt, log = GR.guarded_run(p0, grads, 3e-3, (0.9, 0.999), 1e-8, weight_decay, max_grad_norm=max_norm)
    assert all(abs(a - b['norm']) <= 1e-12 * a for a, b in zip(norms, log))
    if case == 'coef_is_1':
        assert all(e['coef'] == 1.0 for e in log)
    else:
        assert all(e['coef'] < 1.0 for e in log) and abs(log[0]['coef'] - 0.25) < 1e-6
    for i, p in enumerate(params):
        st = opt.state[p]
        assert float(st['step']) == rt[i] == 4
        for name, a, b in (('p', p.detach(), rp[i]), ('exp_avg', st['exp_avg'], rm[i]), ('exp_avg_sq', st['exp_avg_sq'], rv[i])):
            assert ew_err(a, b) < 1e-12, (i, name, ew_err(a, b))


def test_guard_restatement_skips_and_propagates():
    """skip_nonfinite: a NaN or Inf gradient element leaves p, m, v and the step counts of EVERY parameter alone and the following step is step
    t + 1 of the applied ones; without it the NaN goes where torch's clip_grad_norm_ + Adam put it (everywhere, through the NaN coefficient)"""
    g = torch.Generator().manual_seed(22)
    p0 = [torch.randn(5, generator=g), torch.randn(7, generator=g)]
    good = [[torch.randn(5, generator=g), torch.randn(7, generator=g)] for _ in range(2)]
    for bad_value in (float('nan'), float('inf')):
        bad = [good[0][0].clone(), good[0][1].clone()]
        bad[1][-1] = bad_value
        p, m, v, t, log = GR.guarded_run(p0, [good[0], bad, good[1]], 1e-2, skip_nonfinite=True)
        q, mq, vq, tq, _ = GR.guarded_run(p0, good, 1e-2, skip_nonfinite=True)
        assert t == tq == [2, 2] and [e['applied'] for e in log] == [True, False, True] and log[1]['coef'] == 0.0
        assert all(torch.equal(a, b) for a, b in zip(p + m + v, q + mq + vq))
    bad[1][-1] = float('nan')
    p, m, v, t, log = GR.guarded_run(p0, [good[0], bad], 1e-2, max_grad_norm=1.0)
    params = [torch.nn.Parameter(x.clone()) for x in p0]
    opt = torch.optim.Adam(params, lr=1e-2)
    for gs in (good[0], bad):
        for q, gr in zip(params, gs):
            q.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
    assert math.isnan(log[1]['coef']) and all(torch.isnan(x).all() for x in p) and all(torch.isnan(q).all() for q in params)


def test_guard_entry_points_are_declared_and_typed():
    from whmr_amd import _lib as L
    for fn in ('adam_grad_sumsq', 'adam_guard_advance', 'adam_step_guarded'):
        assert callable(getattr(L, fn))
    assert not hasattr(L, 'WhmrAdamGuardCfg') and not hasattr(L, 'WhmrAdamGuardState')          # the ctypes mirrors are private


class _OnDevice(torch.nn.Parameter):
    """a host parameter that answers ``is_cuda`` like a device one: FusedAdam's constructor can be exercised without a GPU (no step is taken)"""
    is_cuda = property(lambda self: True)


def test_fused_adam_validates_max_grad_norm():
    from whmr_amd.train import FusedAdam
    for bad in (0, 0.0, -1.0, float('nan'), float('inf'), -float('inf'), torch.tensor(1.0), '1.0'):
        with pytest.raises(ValueError, match='max_grad_norm'):                     # looked at before the parameters are: a host parameter is enough
            FusedAdam([torch.nn.Parameter(torch.zeros(4))], max_grad_norm=bad)
    opt = FusedAdam([_OnDevice(torch.zeros(4))], max_grad_norm=2, skip_nonfinite=1)
    assert opt.max_grad_norm == 2.0 and isinstance(opt.max_grad_norm, float) and opt.skip_nonfinite is True and opt.guarded
    for bad in (0.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='max_grad_norm'):
            opt.set_grad_guard(max_grad_norm=bad)
        assert opt.max_grad_norm == 2.0
    opt.set_grad_guard(skip_nonfinite=False)
    assert opt.max_grad_norm == 2.0 and opt.skip_nonfinite is False and opt.guarded
    opt.set_grad_guard(max_grad_norm=None)
    assert opt.max_grad_norm is None and not opt.guarded
    with pytest.raises(TypeError):
        FusedAdam([_OnDevice(torch.zeros(4))], max_grad_norm=1.0, norm_type=1.0)     # the L2 norm only: there is no such option


def test_guard_options_stay_out_of_param_groups_and_state_dict():
    """state_dict() interchanges with torch.optim.Adam(capturable=True): the group keys are exactly torch's, guard on or off, and nothing of the
    guard is allocated or counted before a guarded step has run"""
    from whmr_amd.train import FusedAdam
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(4))], capturable=True)
    plain = FusedAdam([_OnDevice(torch.zeros(4))])
    guarded = FusedAdam([_OnDevice(torch.zeros(4))], max_grad_norm=1.0, skip_nonfinite=True)
    assert not plain.guarded and plain.max_grad_norm is None and plain.skip_nonfinite is False
    for opt in (plain, guarded):
        assert set(opt.defaults) == set(ref.defaults)
        assert set(opt.param_groups[0]) == set(ref.param_groups[0])
        sd = opt.state_dict()
        assert set(sd) == {'state', 'param_groups'} and set(sd['param_groups'][0]) == set(ref.state_dict()['param_groups'][0])
        assert opt._guard_state is None and opt._partials is None and opt._guard_cfg is None
        assert opt.guard_summary() == dict(grad_norm=None, clip_coef=None, applied=None, steps_seen=0, steps_skipped=0)
        with pytest.raises(RuntimeError, match='no guarded step'):
            opt.grad_norm
    FusedAdam._check_group(dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0))
