"""Host side of train.FusedAdam (csrc/adam.hip): the float64 restatement the GPU tests compare with is torch's Adam, and the optimizer
refuses what it does not implement instead of falling back."""
import pytest
import torch

import adam_reference as AR
from conftest import ew_err


@pytest.mark.parametrize('weight_decay', [0.0, 0.01])
def test_float64_restatement_is_torch_adam(weight_decay):
    """torch.optim.Adam on float64 CPU parameters, 5 steps: p, exp_avg and exp_avg_sq agree with tests/adam_reference.py to 1e-12 (the two differ
    only in the order of a few float64 roundings)"""
    g = torch.Generator().manual_seed(11)
    shapes = [(1,), (65,), (96, 200), (8, 3, 5, 5)]
    p0 = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    grads = [[torch.randn(s, generator=g, dtype=torch.float64) * (0.1 + k) for s in shapes] for k in range(5)]
    params = [torch.nn.Parameter(x.clone()) for x in p0]
    opt = torch.optim.Adam(params, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    for gs in grads:
        for p, gr in zip(params, gs):
            p.grad = gr.clone()
        opt.step()
    rp, rm, rv, rt = AR.adam_run(p0, grads, 3e-3, (0.9, 0.999), 1e-8, weight_decay)
    for i, p in enumerate(params):
        st = opt.state[p]
        assert float(st['step']) == rt[i] == 5
        for name, a, b in (('p', p.detach(), rp[i]), ('exp_avg', st['exp_avg'], rm[i]), ('exp_avg_sq', st['exp_avg_sq'], rv[i])):
            assert ew_err(a, b) < 1e-12, (i, name, ew_err(a, b))
        assert not torch.equal(p.detach(), p0[i])


def test_a_skipped_gradient_leaves_the_reference_parameter_alone():
    g = torch.Generator().manual_seed(2)
    p0 = [torch.randn(5, generator=g), torch.randn(7, generator=g)]
    grads = [[torch.randn(5, generator=g), torch.randn(7, generator=g)], [None, torch.randn(7, generator=g)]]
    p, m, v, t = AR.adam_run(p0, grads, 1e-2)
    p1, m1, v1, t1 = AR.adam_run(p0, grads[:1], 1e-2)
    assert t == [1, 2] and torch.equal(p[0], p1[0]) and torch.equal(m[0], m1[0]) and torch.equal(v[0], v1[0]) and not torch.equal(p[1], p1[1])


def test_fused_adam_refuses_what_it_does_not_implement():
    from whmr_amd.train import FusedAdam
    with pytest.raises(ValueError, match='no CPU fallback'):
        FusedAdam([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(ValueError, match='fp32'):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))])
    # each flag is refused for itself: the message names that flag alone, and the flags are looked at before the parameters are (a host parameter,
    # refused above, would otherwise raise the same exception type)
    for flag in ('amsgrad', 'maximize', 'differentiable'):
        with pytest.raises(ValueError) as e:
            FusedAdam([torch.nn.Parameter(torch.zeros(4))], **{flag: True})
        assert str(e.value) == 'FusedAdam implements plain Adam only: %s is not supported' % flag
    for flag in ('amsgrad', 'maximize', 'differentiable', 'decoupled_weight_decay'):          # ... and in a group, e.g. one a loaded state_dict brought
        group = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, **{flag: True})
        with pytest.raises(ValueError) as e:
            FusedAdam._check_group(group)
        assert str(e.value) == 'FusedAdam implements plain Adam only: %s is not supported' % flag
    FusedAdam._check_group(dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False))
    with pytest.raises(ValueError):
        FusedAdam([torch.nn.Parameter(torch.zeros(4))], lr=torch.tensor(1e-3))


def test_adam_entry_points_are_exported_and_public_names_stay_put():
    from whmr_amd import _lib as L
    from whmr_amd import train
    assert not hasattr(L, 'WhmrAdamItem') and not hasattr(L, 'WhmrAdamHyper')          # the ctypes mirrors are private
    assert hasattr(L.WeightOperands, 'mark_current')
    assert train.FusedAdam.__module__ == 'whmr_amd.train.optim' and callable(train.capture_update_step)
