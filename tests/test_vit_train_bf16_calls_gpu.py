"""Every library call of one bf16 ViT training step (forward + backward), checked against its float64 reference (tests/bf16_reference.py) with
the bound derived from the kernel's own arithmetic.  A recorder (tests/call_recorder.py) wraps every public function of ``whmr_amd._lib``: each top-level call is
snapshotted (inputs cloned on the current stream), run, and checked right away; a call with no reference, or with a flag its reference does
not model, fails the test, and the number of calls of each kind is asserted per configuration."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_reference as R  # noqa: E402
import call_recorder  # noqa: E402

pytestmark = pytest.mark.gpu


class Recorder(call_recorder.Recorder):
    # ------------------------------------------------------------------------------------------------------------- one handler per call
    def on_patch_im2col(self, live, s):
        self._only(live, {'x', 'out', 'patch', 'pad'}, self.sigs['patch_im2col'].parameters)
        want = R.patch_im2col(s['x'], s['patch'], s['pad'], live['out'].dtype)
        assert torch.equal(live['out'], want.view_as(live['out'])), 'patch_im2col differs from the exact gather'
        self.counts['patch_im2col bit-exact'] += 1

    def on_gemm(self, live, s):
        L = self.L
        self._only(live, {'a', 'w', 'out', 'bias', 'residual', 'res_row_mod', 'act', 'pre_out', 'gelu_bwd_of', 'row_scale'},
                   self.sigs['gemm'].parameters)
        a, w, out = s['a'], s['w'], live['out']
        assert a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16, 'bf16 step: GEMM operands must be bf16'
        if live['gelu_bwd_of'] is not None:
            assert live['bias'] is None and live['residual'] is None and live['row_scale'] is None and live['act'] == L.ACT_NONE
            r, m, alpha = R.gemm_gelu_bwd(a, w, s['gelu_bwd_of'])
            self.record('gemm dX * gelu\'(pre) (bf16)', R.check(out, r, m, n_round=R.N_ROUND_GEMM_GELU_BWD, alpha=alpha))
            return
        if live['pre_out'] is not None:
            assert live['act'] == L.ACT_GELU and live['residual'] is None and live['row_scale'] is None
            r, m = R.gemm(a, w, bias=s['bias'])
            self.record('gemm fc1 pre-activation (bf16)', R.check(live['pre_out'], r, m))
            gz = R.gelu(live['pre_out'])                                     # GELU of the stored bf16 z: one rounding + gelu_fast's error
            self.record('gemm fc1 GELU of the stored pre (bf16)', R.check(out, gz, torch.zeros_like(gz), alpha=R.GELU_ABS))
            return
        assert live['act'] == L.ACT_NONE, 'activation %r without pre_out is not modelled' % live['act']
        r, m = R.gemm(a, w, bias=s['bias'], residual=s['residual'], res_row_mod=live['res_row_mod'], row_scale=s['row_scale'])
        if live['res_row_mod']:
            assert live['row_scale'] is None
            key = 'gemm patch + bias + pos (fp32)'
        elif live['row_scale'] is not None:
            key = 'gemm + bias + residual, row_scale (fp32)'
        elif live['residual'] is not None:
            key = 'gemm + bias + residual (fp32)'
        elif live['bias'] is not None:
            key = 'gemm + bias (%s)' % ('bf16' if out.dtype == torch.bfloat16 else 'fp32')
        else:
            key = 'gemm dX (%s)' % ('bf16' if out.dtype == torch.bfloat16 else 'fp32')
        self.record(key, R.check(out, r, m))

    def on_layernorm(self, live, s):
        r, m = R.layernorm(s['x'], s['weight'], s['bias'], live['eps'])
        self.record('layernorm (%s)' % ('bf16' if live['out'].dtype == torch.bfloat16 else 'fp32'), R.check(live['out'], r, m))

    def on_attention_fwd_train(self, live, s):
        B, N, H, d, sc = (live[k] for k in ('B', 'N', 'H', 'd', 'scale'))
        (ro, mo), (rl, ml) = R.attention_fwd(s['qkv'], B, N, H, d, sc)
        self.record('attention_fwd_train o (bf16)', R.check(live['out'], ro, mo, n_round=R.N_ROUND_ATT_FWD))
        self.record('attention_fwd_train lse (fp32)', R.check(live['lse'], rl, ml))

    def on_attention_bwd(self, live, s):
        B, N, H, d, sc = (live[k] for k in ('B', 'N', 'H', 'd', 'scale'))
        r, m = R.attention_bwd(s['qkv'], s['o'], s['dout'], s['lse'], B, N, H, d, sc)
        nr = R.attention_bwd_n_round(B, N, H, d, r.device)
        self.record('attention_bwd dqkv (bf16)', R.check(live['dqkv'], r, m, n_round=nr))

    def on_layernorm_bwd(self, live, s):
        acc = live['accumulate']
        ref = R.layernorm_bwd(s['x'], s['dy'], s['gamma'], live['eps'], dres=s['dres'],
                              dgamma_prior=s['dgamma'] if acc else None, dbeta_prior=s['dbeta'] if acc else None)
        tag = ' (dres%s)' % (' = dx' if live['dres'] is not None and live['dres'].data_ptr() == live['dx'].data_ptr() else
                             '' if live['dres'] is not None else ' none')
        self.record('layernorm_bwd dx' + tag, R.check(live['dx'], *ref['dx']))
        self.record('layernorm_bwd dgamma', R.check(live['dgamma'], *ref['dgamma'], kappa=R.KAPPA_SUM))
        self.record('layernorm_bwd dbeta', R.check(live['dbeta'], *ref['dbeta'], kappa=R.KAPPA_SUM))
        if live['cast_out'] is not None:
            want = R.cast_rows(live['dx'], live['row_scale'])
            assert torch.equal(live['cast_out'], want.view_as(live['cast_out'])), 'cast_out != bf16(dx * row_scale)'
            self.counts['layernorm_bwd cast_out bit-exact'] += 1
            if live['row_scale'] is not None:
                self.counts['layernorm_bwd cast_out with row_scale'] += 1

    def _tn(self, key, a, b, out, db_live):
        if db_live is None:
            r, m = R.gemm_tn(a, b)
        else:
            (r, m), (rd, md) = R.gemm_tn(a, b, db=True)
            self.record(key + ' db', R.check(db_live, rd, md, kappa=R.KAPPA_SUM))
        self.record(key + ' dW', R.check(out, r, m, kappa=R.KAPPA_SUM))

    def on_gemm_tn(self, live, s):
        self._only(live, {'a', 'b', 'out', 'db'}, self.sigs['gemm_tn'].parameters)
        self._tn('gemm_tn', s['a'], s['b'], live['out'], live['db'])

    def on_gemm_tn_group(self, live, s):
        for (a, b, _, _), (_, _, out, db) in zip(s['jobs'], live['jobs']):
            self._tn('gemm_tn_group', a, b, out, db)

    def on_colsum(self, live, s):
        r, m = R.colsum(s['x'], s['out'] if live['accumulate'] else None)
        self.record('colsum (dpos)', R.check(live['out'], r, m, kappa=R.KAPPA_SUM))


CONFIGS = {
    # name: (img size, batch, embed dim, heads, depth, drop_path_rate)
    'vitb_256x192_b64_d3': ((256, 192), 64, 768, 12, 3, 0.3),
    'vitb_224_b64_d1': ((224, 224), 64, 768, 12, 1, 0.0),
    'vitl_256x192_b32_d2': ((256, 192), 32, 1024, 16, 2, 0.5),
}


@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_vit_bf16_training_step_bf16_calls_vs_float64(dev, cfg, monkeypatch):
    from oracle import synth
    from whmr_amd import _lib as L
    from whmr_amd.models.pose_vit import ViT
    size, B, D, H, depth, rate = CONFIGS[cfg]
    sd = synth.make_vit_state(21, size, embed_dim=D, depth=depth)
    x = synth.make_inputs(B, 22, size)['x'].to(dev)
    m = ViT(img_size=size, embed_dim=D, depth=depth, num_heads=H, qkv_bias=True, numerics='bf16', drop_path_rate=rate)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train()
    # stochastic depth: in every block with dpr > 0, samples b % 3 == 1 drop the attention branch and b % 3 == 2 the MLP branch
    masks = torch.ones(2 * depth, B)
    for i in range(depth):
        if m.dpr[i] > 0:
            masks[2 * i, 1::3] = 0
            masks[2 * i + 1, 2::3] = 0
    m.drop_masks = masks
    P = m.patch_size
    Hp, Wp = (size[0] + 2 * m.patch_pad - P) // P + 1, (size[1] + 2 * m.patch_pad - P) // P + 1
    N, M = Hp * Wp, B * Hp * Wp
    G = torch.randn(B, D, Hp, Wp, generator=torch.Generator().manual_seed(23)).to(dev)
    rec = Recorder(L)
    rec.install(monkeypatch)
    torch.cuda.reset_peak_memory_stats(dev)
    (m(x) * G).sum().backward()
    torch.cuda.synchronize(dev)
    monkeypatch.undo()
    peak = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    nd = sum(1 for p in m.dpr if p > 0)
    want = {'patch_im2col': 1, 'patch_im2col bit-exact': 1,
            'gemm': 1 + 4 * depth + 4 * depth,                          # patch + 4 per block forward, 4 data gradients per block
            'layernorm': 2 * depth + 1, 'attention_fwd_train': depth, 'attention_bwd': depth,
            'layernorm_bwd': 2 * depth + 1, 'layernorm_bwd cast_out bit-exact': 2 * depth + 1,
            'layernorm_bwd cast_out with row_scale': 2 * nd,
            'gemm_tn_group': depth, 'gemm_tn': 1, 'colsum': 1}
    got = {k: v for k, v in rec.counts.items() if v}
    assert got == {k: v for k, v in want.items() if v}, (got, want)
    # WeightOperands (one whmr_weights_prepare launch): the W and W^T copies are the single bf16 rounding of the fp32 weights
    wo = m._train_operands
    for p in wo.params:
        w, wt = wo.copies[id(p)]
        assert torch.equal(w, p.detach().reshape(w.shape).bfloat16()) and torch.equal(wt, w.t()), 'WeightOperands copy differs from bf16(W)'
    for p in m.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    print('\n[%s] M = %d, N = %d, peak %.1f GiB; worst error / allowance per op:' % (cfg, M, N, peak))
    for k in sorted(rec.worst):
        print('  %-48s %.3e' % (k, rec.worst[k]))
