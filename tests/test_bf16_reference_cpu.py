"""The float64 references and the derived-bound checker of tests/bf16_reference.py on small CPU tensors: exact (and kernel-like rounded) results
pass, and each of a set of subtle kernel faults fails -- so the checker cannot quietly become permissive."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_reference as R  # noqa: E402


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bf(t):
    return t.to(torch.bfloat16).double()


def test_exact_results_pass_and_a_4x_allowance_shift_fails():
    g = _g(0)
    a = torch.randn(64, 256, generator=g).bfloat16()
    w = (torch.randn(96, 256, generator=g) * 0.05).bfloat16()
    b = torch.randn(96, generator=g)
    r, m = R.gemm(a, w, bias=b)
    assert R.check(r.float(), r, m) <= 1.0
    assert R.check(r.bfloat16(), r, m) <= 1.0                                          # one RNE to the bf16 output
    y = r.clone()
    allow = R.RHO_F32 * r[5, 7].abs() + R.KAPPA * m[5, 7]
    y[5, 7] += 4 * allow
    assert R.check(y, r, m, rho_out=R.RHO_F32) > 3.9
    assert R.check(y.float(), r, m) > 1.0
    nan = r.float().clone()
    nan[0, 0] = float('nan')
    assert R.check(nan, r, m) == math.inf


@pytest.mark.parametrize('out_dtype', [torch.float32, torch.bfloat16])
def test_gemm_missing_one_k_slice_fails(out_dtype):
    """K = 2048: a kernel that skips one 32-row K slice (k 1024..1055) for the whole output"""
    g = _g(1)
    a = torch.randn(128, 2048, generator=g).bfloat16()
    w = (torch.randn(64, 2048, generator=g) * 0.03).bfloat16()
    r, m = R.gemm(a, w)
    good = (a.float() @ w.float().t()).to(out_dtype)                                   # fp32 accumulation + the output rounding
    assert R.check(good, r, m) <= 1.0
    keep = torch.ones(2048, dtype=torch.bool)
    keep[1024:1056] = False
    bad = (a.float()[:, keep] @ w.float()[:, keep].t()).to(out_dtype)
    assert R.check(bad, r, m) > 1.0


def test_row_scale_on_the_wrong_rows_fails():
    """fp32 out = residual + row_scale[m] (a . w^T + bias) (stochastic depth): the factors of two samples swapped"""
    g = _g(2)
    M, N = 4 * 48, 128
    a = torch.randn(M, 256, generator=g).bfloat16()
    w = (torch.randn(N, 256, generator=g) * 0.05).bfloat16()
    b, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    rs = torch.tensor([0.0, 1 / 0.7, 1 / 0.7, 0.0]).repeat_interleave(48)
    r, m = R.gemm(a, w, bias=b, residual=res, row_scale=rs)
    br = (a.float() @ w.float().t() + b)
    assert R.check(res + rs.view(-1, 1) * br, r, m) <= 1.0
    wrong = rs.view(4, 48)[[1, 0, 2, 3]].reshape(-1)
    assert R.check(res + wrong.view(-1, 1) * br, r, m) > 1.0
    # the position-embedding residual of the patch GEMM: rows m % res_row_mod
    pos = torch.randn(48, N, generator=g)
    r2, m2 = R.gemm(a, w, bias=b, residual=pos, res_row_mod=48)
    assert R.check(br + pos.repeat(4, 1), r2, m2) <= 1.0
    assert R.check(br + pos.roll(1, 0).repeat(4, 1), r2, m2) > 1.0


def _attention_inputs(B, N, H, d, seed, amp=1.5):
    g = _g(seed)
    qkv = (torch.randn(B * N, 3 * H * d, generator=g) * amp).bfloat16()
    dout = torch.randn(B * N, H * d, generator=g)
    return qkv, dout


def _kernel_like_attention(qkv, dout, lse, B, N, H, d, scale):
    """fp32 arithmetic with the roundings the MFMA kernels do by design: P -> bf16 for P.V (forward); dO, P, dS -> bf16 (backward)"""
    q, k, v = qkv.float().view(B, N, 3, H, d).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    o = (e.bfloat16().float() @ v) / e.sum(-1, keepdim=True)
    o = o.transpose(1, 2).reshape(B * N, H * d).bfloat16()
    ls = lse.view(B, H, N, 1)
    p = torch.exp2(s * (1 / math.log(2)) - ls)
    do = dout.view(B, N, H, d).transpose(1, 2)
    D = (do * o.float().view(B, N, H, d).transpose(1, 2)).sum(-1, keepdim=True)
    dp = do.bfloat16().float() @ v.transpose(-1, -2)
    ds = (scale * p * (dp - D)).bfloat16().float()
    dq, dk = ds @ k, ds.transpose(-1, -2) @ q
    dv = p.bfloat16().float().transpose(-1, -2) @ do.bfloat16().float()
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * d).bfloat16()
    return o, dqkv


@pytest.mark.parametrize('N,amp', [(97, 1.5), (65, 4.0)])
def test_attention_references_pass_the_designed_roundings_and_catch_a_shifted_lse(N, amp):
    B, H, d = 2, 2, 64
    scale = d ** -0.5
    qkv, dout = _attention_inputs(B, N, H, d, N, amp)
    (o_r, o_m), (l_r, l_m) = R.attention_fwd(qkv, B, N, H, d, scale)
    lse = l_r.float()
    o, dqkv = _kernel_like_attention(qkv, dout, lse, B, N, H, d, scale)
    assert R.check(o, o_r, o_m, n_round=R.N_ROUND_ATT_FWD) <= 1.0
    assert R.check(lse, l_r, l_m) <= 1.0
    r, m = R.attention_bwd(qkv, o, dout, lse, B, N, H, d, scale)
    nr = R.attention_bwd_n_round(B, N, H, d, r.device)
    assert R.check(dqkv, r, m, n_round=nr) <= 1.0
    # without the modelled roundings the bound is not met by construction: the roundings of dqkv are what n_round counts
    assert R.check(dqkv, r, m, n_round=0) > R.check(dqkv, r, m, n_round=nr)
    # an lse off by 2^-8 (log2 units) -- what a wrong log2 / ln 2 conversion or a dropped key in the row sum leaves -- fails the lse check
    assert R.check(lse + 2.0 ** -8, l_r, l_m) > 1.0
    # and a backward fed the float64 lse in natural-log units (the log2-domain contract broken) fails the dqkv check
    _, bad = _kernel_like_attention(qkv, dout, (l_r * R.LN2).float(), B, N, H, d, scale)
    assert R.check(bad, r, m, n_round=nr) > 1.0


def _layernorm_inputs(rows, C, seed):
    g = _g(seed)
    x = torch.randn(rows, C, generator=g) + 30.0
    x[:, 5] *= 8.0
    return x, torch.randn(rows, C, generator=g), torch.randn(C, generator=g), torch.randn(rows, C, generator=g)


def test_layernorm_bwd_reference_and_a_missing_block_partial():
    """rows = 4096: the kernel's 1024 workgroups of 4 rows each; a dgamma / dbeta without one workgroup's partial must fail"""
    rows, C = 4096, 64
    x, dy, gam, dres = _layernorm_inputs(rows, C, 3)
    ref = R.layernorm_bwd(x, dy, gam, 1e-6, dres=dres)
    xt = x.clone().requires_grad_(True)
    gt, bt = gam.clone().requires_grad_(True), torch.zeros(C, requires_grad=True)
    torch.nn.functional.layer_norm(xt, (C,), gt, bt, 1e-6).backward(dy)
    assert R.check(xt.grad + dres, *ref['dx']) <= 1.0                                 # fp32 autograd is within the fp32 bound
    assert R.check(gt.grad, *ref['dgamma'], kappa=R.KAPPA_SUM) <= 1.0 and R.check(bt.grad, *ref['dbeta'], kappa=R.KAPPA_SUM) <= 1.0
    mu = x.double().mean(-1, keepdim=True)
    xh = (x.double() - mu) * ((x.double() - mu).pow(2).mean(-1, keepdim=True) + 1e-6).rsqrt()
    part_g = (dy.double() * xh).view(1024, 4, C).sum(1).float()                        # per-workgroup partials (fp32)
    part_b = dy.view(1024, 4, C).sum(1)
    assert R.check(part_g.sum(0), *ref['dgamma'], kappa=R.KAPPA_SUM) <= 1.0 and R.check(part_b.sum(0), *ref['dbeta'], kappa=R.KAPPA_SUM) <= 1.0
    assert R.check(part_g[1:].sum(0), *ref['dgamma'], kappa=R.KAPPA_SUM) > 1.0
    assert R.check(part_b[:-1].sum(0), *ref['dbeta'], kappa=R.KAPPA_SUM) > 1.0
    # accumulate: prior values are part of the result
    prior = torch.randn(C, generator=_g(4))
    acc = R.layernorm_bwd(x, dy, gam, 1e-6, dgamma_prior=prior, dbeta_prior=prior)
    assert R.check(prior + part_g.sum(0), *acc['dgamma'], kappa=R.KAPPA_SUM) <= 1.0
    assert R.check(part_g.sum(0), *acc['dgamma'], kappa=R.KAPPA_SUM) > 1.0
    # cast_out is a single rounding of the kernel's own dx: equal or not
    rs = torch.tensor([0.0, 2.0]).repeat(rows // 2)
    y = R.cast_rows(xt.grad, rs)
    assert torch.equal(y[0::2].float(), torch.zeros(rows // 2, C)) and torch.equal(y[1::2], (xt.grad[1::2] * 2).bfloat16())


def test_forward_layernorm_gelu_and_small_ops():
    g = _g(5)
    x, _, gam, _ = _layernorm_inputs(33, 216, 6)
    bet = torch.randn(216, generator=g)
    r, m = R.layernorm(x, gam, bet, 1e-6)
    y = torch.nn.functional.layer_norm(x, (216,), gam, bet, 1e-6)
    assert R.check(y, r, m) <= 1.0 and R.check(y.bfloat16(), r, m) <= 1.0
    xc = torch.randn(33, 216, generator=g)                                             # (x's +30 row mean and outlier are in m: the fp32 kernel cancels them)
    rc, mc = R.layernorm(xc, gam, bet, 1e-6)
    assert R.check(torch.nn.functional.layer_norm(xc, (216,), gam, bet, 1e-3), rc, mc) > 1.0    # another eps
    # GELU of the stored pre-activation: exact-erf reference, gelu_fast within GELU_ABS
    z = (torch.randn(4096, generator=g) * 3).bfloat16()
    gr = R.gelu(z)
    tanh_form = torch.nn.functional.gelu(z.float(), approximate='tanh')                  # 4.7e-4 off: outside the documented bound
    assert R.check(torch.nn.functional.gelu(z.float()).bfloat16(), gr, torch.zeros_like(gr), alpha=R.GELU_ABS) <= 1.0
    assert R.check(tanh_form, gr, torch.zeros_like(gr), alpha=R.GELU_ABS, rho_out=0.0) > 1.0
    # fc2's data gradient times gelu'(z): accumulator staged as bf16, then the product rounded
    a = torch.randn(64, 256, generator=g).bfloat16()
    w = (torch.randn(128, 256, generator=g) * 0.05).bfloat16()
    zz = (torch.randn(64, 128, generator=g) * 2).bfloat16()
    r, m, alpha = R.gemm_gelu_bwd(a, w, zz)
    lin = (a.float() @ w.float().t()).bfloat16().float()
    dg = R.gelu_grad(zz).float()
    assert R.check((lin * dg).bfloat16(), r, m, n_round=R.N_ROUND_GEMM_GELU_BWD, alpha=alpha) <= 1.0
    assert R.check((lin * 0.5).bfloat16(), r, m, n_round=R.N_ROUND_GEMM_GELU_BWD, alpha=alpha) > 1.0      # gelu' dropped
    # TN weight gradient with its bias column sums; colsum
    ka = torch.randn(256, 64, generator=g).bfloat16()
    kb = torch.randn(256, 256, generator=g).bfloat16()
    (r, m), (rd, md) = R.gemm_tn(ka, kb, db=True)
    assert R.check(ka.float().t() @ kb.float(), r, m, kappa=R.KAPPA_SUM) <= 1.0 and R.check(ka.float().sum(0), rd, md, kappa=R.KAPPA_SUM) <= 1.0
    assert R.check(ka.float()[32:].t() @ kb.float()[32:], r, m, kappa=R.KAPPA_SUM) > 1.0
    xs = torch.randn(64, 300, generator=g)
    r, m = R.colsum(xs)
    assert R.check(xs.sum(0), r, m, kappa=R.KAPPA_SUM) <= 1.0 and R.check(xs[1:].sum(0), r, m, kappa=R.KAPPA_SUM) > 1.0
    # patch gather: columns (c, ky, kx), zero padding
    img = torch.randn(2, 3, 36, 20, generator=g)
    cols = R.patch_im2col(img, 16, 2, torch.bfloat16)
    assert cols.shape == (2 * 2 * 1, 3 * 256)
    assert torch.equal(cols[0].view(3, 16, 16)[:, 2:, 2:], img[0, :, :14, :14].bfloat16())
    assert not cols[0].view(3, 16, 16)[:, :2].any()
