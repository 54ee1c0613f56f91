"""Host side of train.FusedAdam (csrc/adam.hip): the float64 restatement the GPU tests compare with is torch's Adam, the ctypes mirrors and the
packed table rows have the C header's layout, and the optimizer refuses what it does not implement instead of falling back."""
import ctypes
import os
import subprocess

import pytest
import torch

import adam_reference as AR
from conftest import ROOT, ew_err


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


def test_adam_structs_match_the_c_header_layout(tmp_path):
    """struct whmr_adam_item / whmr_adam_hyper: size and field offsets of the ctypes mirrors equal gcc's for include/whmr_hip.h, WHMR_ADAM_CHUNK equals
    the Python constant, and the struct format train/optim.py packs table rows with puts every field where the mirror has it"""
    from whmr_amd import _lib as L
    from whmr_amd.train import optim
    pairs = {'whmr_adam_item': L._WhmrAdamItem, 'whmr_adam_hyper': L._WhmrAdamHyper}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "whmr_hip.h"', 'int main(void) {', '  printf("chunk %d\\n", WHMR_ADAM_CHUNK);']
    for cname, cls in pairs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(struct %s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(struct %s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['chunk']) == L.ADAM_CHUNK
    for cname, cls in pairs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), (cname, got[cname], ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(cls, fname).offset, (cname, fname)
    names = [f for f, _ in L._WhmrAdamItem._fields_]
    values = [0x1000 * (i + 1) for i in range(8)] + [11, 12, 13, 14, 15, 16, 0.1, 0.001]
    assert len(values) == len(names)
    row = L._WhmrAdamItem.from_buffer_copy(optim._ITEM.pack(*values))
    assert [getattr(row, f) for f in names] == values
    hyper = L._WhmrAdamHyper.from_buffer_copy(optim._HYPER.pack(0.9, 0.999, 5e-5, 0.5, 0.125))
    assert (hyper.beta1, hyper.beta2, hyper.lr, hyper.eps, hyper.weight_decay) == (0.9, 0.999, 5e-5, 0.5, 0.125)       # betas and lr: doubles, kept exactly


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
    assert 'whmr_adam_advance' in L.EXPORTS and 'whmr_adam_step' in L.EXPORTS
    assert not hasattr(L, 'WhmrAdamItem') and not hasattr(L, 'WhmrAdamHyper')          # the ctypes mirrors are private
    assert hasattr(L.WeightOperands, 'mark_current')
    assert train.FusedAdam.__module__ == 'whmr_amd.train.optim' and callable(train.capture_update_step)
    hdr = open(os.path.join(ROOT, 'include', 'whmr_hip.h')).read()
    assert 'int whmr_adam_advance(' in hdr and 'int whmr_adam_step(' in hdr
