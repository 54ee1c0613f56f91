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


# ------------------------------------------------------------------------------------------------ blocked bf16 inference path
# fp32 emulations of the kernels' arithmetic with their designed roundings (csrc/gemm_blk16_impl.h, attention_blk16.hip) must pass; each of a
# set of subtle faults must fail.  M = 70 ends inside a 32-row block; C = 512 gives two 256-column statistics partials per row.

def _fold_case(seed=11, M=70, C=512, N2=256, K0=64, mean_in_std=20.0, std=2.0):
    g = _g(seed)
    att = torch.randn(M, K0, generator=g).bfloat16()
    wp = (torch.randn(C, K0, generator=g) / math.sqrt(K0)).bfloat16()
    bp = torch.randn(C, generator=g)
    t1 = torch.randn(M, C, generator=g) * std + mean_in_std * std * torch.sign(torch.randn(M, 1, generator=g))
    t0 = t1 - (att.float() @ wp.float().t() + bp)                        # the stream before the producer, which re-creates t1
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1, torch.randn(C, generator=g) * 0.2
    w2 = torch.randn(N2, C, generator=g) / math.sqrt(C)
    b2 = torch.randn(N2, generator=g)
    wf = (w2 * gamma).bfloat16()
    return dict(M=M, C=C, att=att, wp=wp, bp=bp, t0=t0, wf=wf, wf_exact=w2 * gamma, colsum=wf.float().sum(1), c=b2 + w2 @ beta)


def _emu_producer(k, shift=None, shift_stats=None, sums_of_shifted=True):
    """gemm_blk16_impl.h:276-299, 327-369 in fp32 -> (C, s, xhat, stats [M, C/256, 2])"""
    M, C = k['M'], k['C']
    t = k['att'].float() @ k['wp'].float().t() + k['bp'] + k['t0']
    s = torch.zeros(M) if shift is None else shift.clone()
    if shift_stats is not None:
        s = shift_stats[:, :, 0].sum(1) * (1.0 / C) + s
    o = t - s.view(-1, 1)
    q = (o if sums_of_shifted else t).view(M, C // 256, 256)
    return t, s, o.bfloat16(), torch.stack([q.sum(-1), (q * q).sum(-1)], -1)


def _emu_consumer(xhat, k, stats, colsum=None, gelu=False, eps=1e-6):
    """gemm_blk16_impl.h:216-256 in fp32: one-pass variance from the partial sums, rstd * acc + (c - rstd * mean * colsum), one rounding"""
    K = xhat.shape[1]
    colsum = k['colsum'] if colsum is None else colsum
    mean = stats[:, :, 0].sum(1) / K
    var = (stats[:, :, 1].sum(1) / K - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    v = (xhat.float() @ k['wf'].float().t()) * rstd.view(-1, 1) + (k['c'] - (rstd * mean).view(-1, 1) * colsum)
    if gelu:
        v = torch.nn.functional.gelu(v)
    return v.bfloat16()


def _ratio_consumer(y, xhat, k, stats, colsum=None, epi=R.EPI_BF16):
    colsum = k['colsum'] if colsum is None else colsum
    r, m, alpha, kappa, amp = R.fold_consumer(R.block(xhat), R.block(k['wf']), k['M'], stats, colsum, k['c'], 1e-6, epi)
    return R.check(y, r, m, alpha=alpha, kappa=kappa), amp.max().item()


def _ratio_semantic(y, t, s, k, epi=R.EPI_BF16):
    r, m, alpha, kappa, amp = R.fold_semantic(R.block(t), s, k['M'], R.block(k['wf']), k['c'], 1e-6, epi)
    return R.check(y, r, m, alpha=alpha, kappa=kappa), amp.max().item()


def test_blocked_layout_helpers_and_gemm_blk_epilogues():
    g = _g(20)
    x = torch.randn(70, 64, generator=g)
    assert R.block(x).shape == (3, 16, 32, 4) and R.block(x.bfloat16()).shape == (3, 8, 32, 8)
    assert R.block(x)[1, 3, 5, 2] == x[37, 14] and torch.equal(R.unblock(R.block(x), 70), x) and not R.unblock(R.block(x), 96)[70:].any()
    M, N, K = 70, 256, 96                                                 # K = 3 half tiles of 32
    a = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16()
    bias, res, pos = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(12, N, generator=g)
    ab, wb = R.block(a), R.block(w)
    lin = a.float() @ w.float().t() + bias
    rows = torch.arange(M)
    for epi, good, kw in ((R.EPI_BF16, lin.bfloat16(), {}),
                          (R.EPI_BF16_GELU, torch.nn.functional.gelu(lin).bfloat16(), {}),
                          (R.EPI_F32_RES, lin + res, dict(res=R.block(res))),
                          (R.EPI_F32_POS, lin + pos[rows % 12], dict(res=pos, res_rows=12))):
        r, m, alpha = R.gemm_blk(ab, wb, M, bias=bias, epi=epi, **kw)
        assert R.check(good, r, m, alpha=alpha) <= 1.0, epi
    # one 32-deep K half tile dropped (k 32..63)
    keep = torch.ones(K, dtype=torch.bool)
    keep[32:64] = False
    r, m, alpha = R.gemm_blk(ab, wb, M, bias=bias)
    assert R.check((a.float()[:, keep] @ w.float()[:, keep].t() + bias).bfloat16(), r, m) > 1.0
    # EPI_F32_POS with row m % (res_rows + 1) of a table that has the extra row
    pos13 = torch.randn(13, N, generator=g)
    r, m, alpha = R.gemm_blk(ab, wb, M, bias=bias, epi=R.EPI_F32_POS, res=pos13, res_rows=12)
    assert R.check(lin + pos13[rows % 12], r, m) <= 1.0 and R.check(lin + pos13[rows % 13], r, m) > 1.0
    # the erf GELU shifted by 5e-4 (2.6 x the documented error of gelu_fast); no output rounding, so that the shift is all there is
    r, m, alpha = R.gemm_blk(ab, wb, M, bias=bias, epi=R.EPI_BF16_GELU)
    ge = torch.nn.functional.gelu(lin.double())
    assert R.check(ge, r, m, alpha=alpha, rho_out=0.0) <= 1.0 and R.check(ge + 5e-4, r, m, alpha=alpha, rho_out=0.0) > 1.0


@pytest.mark.parametrize('form', ['none', 'shift', 'shift+stats'])
def test_fold_pair_emulation_passes_both_forms(form):
    k = _fold_case()
    M, C = k['M'], k['C']
    if form == 'none':
        k = _fold_case(mean_in_std=0.3)                                   # without a shift only a nearly centred stream meets the condition
        shift = stats_prev = None
    else:
        # the chain: s = the row means one residual step earlier; with 'shift+stats' they arrive as an older shift + the means of the sums taken
        # relative to it
        mu0 = k['t0'].mean(1)
        shift = mu0 if form == 'shift' else mu0 - 0.25
        stats_prev = None if form == 'shift' else torch.stack([(k['t0'] - shift.view(-1, 1)).view(M, C // 256, 256).sum(-1),
                                                               torch.zeros(M, C // 256)], -1)
    t, s, xhat, stats = _emu_producer(k, shift, stats_prev)
    p = R.fold_producer(R.block(t), M, shift=shift, shift_stats=stats_prev, shift_out=s if form != 'none' else None)
    if form == 'none':
        assert p['s'] is None and not p['s_live'].any()
    else:
        assert R.check(s, *p['s'], rho_out=R.RHO_F32) <= 1.0 and R.check(s + 1e-2, *p['s'], rho_out=R.RHO_F32) > 1.0
    assert torch.equal(p['xhat'], xhat)
    assert R.check(stats, *p['stats']) <= 1.0
    for gelu, epi in ((False, R.EPI_BF16), (True, R.EPI_BF16_GELU)):
        y = _emu_consumer(xhat, k, stats, gelu=gelu)
        rc, amp_c = _ratio_consumer(y, xhat, k, stats, epi=epi)
        rs, amp_s = _ratio_semantic(y, t, s, k, epi=epi)
        assert amp_c <= R.AMP_MAX and amp_s <= R.AMP_MAX, (amp_c, amp_s)              # 1.0 with a shift, 1.25 without (mean 0.3 std)
        assert rc <= 1.0 and rs <= 1.0, (form, gelu, rc, rs)
    assert R.check(k['colsum'], *R.fold_colsum(R.block(k['wf'])), kappa=R.KAPPA_SUM) <= 1.0


def test_fold_faults_are_rejected():
    k = _fold_case()
    M, C = k['M'], k['C']
    shift = k['t0'].mean(1)
    t, s, xhat, stats = _emu_producer(k, shift)
    y = _emu_consumer(xhat, k, stats)
    assert _ratio_consumer(y, xhat, k, stats)[0] <= 1.0 and _ratio_semantic(y, t, s, k)[0] <= 1.0
    # a consumer that misses one 256-column statistics partial
    half = stats.clone()
    half[:, 1] = 0
    assert _ratio_consumer(_emu_consumer(xhat, k, half), xhat, k, stats)[0] > 1.0
    # a consumer reading the statistics of a different stream (a stale buffer): correct for the inputs it got, wrong for the model
    other = _fold_case(seed=12, std=3.0)
    _, _, _, stale = _emu_producer(other, other['t0'].mean(1))
    y_stale = _emu_consumer(xhat, k, stale)
    rc, amp_c = _ratio_consumer(y_stale, xhat, k, stale)
    rs, amp_s = _ratio_semantic(y_stale, t, s, k)
    assert amp_c <= R.AMP_MAX and amp_s <= R.AMP_MAX
    assert rc <= 1.0 < rs, (rc, rs)
    # a producer whose bf16 copy is shifted but whose sums are not: its own statistics check fails, and so does the pair's meaning
    _, _, xh2, raw = _emu_producer(k, shift, sums_of_shifted=False)
    assert torch.equal(xh2, xhat)
    assert R.check(raw, *R.fold_producer(R.block(t), M, shift=shift, shift_out=s)['stats']) > 1.0
    assert _ratio_semantic(_emu_consumer(xhat, k, raw), t, s, k)[0] > 1.0
    # colsum taken from the unrounded gamma o W: the mean term no longer cancels against what the MFMAs multiply
    assert R.check(k['wf_exact'].sum(1), *R.fold_colsum(R.block(k['wf'])), kappa=R.KAPPA_SUM) > 1.0
    # the amplification guard: a row at |mean| = 20 std WITHOUT a shift is far outside the condition (amp = 1 + 2 * 400)
    _, _, xraw, sraw = _emu_producer(k)
    amp = R.fold_consumer(R.block(xraw), R.block(k['wf']), M, sraw, k['colsum'], k['c'], 1e-6)[4]
    assert amp.min() > 100 * R.AMP_MAX
    with pytest.raises(AssertionError, match='amplification'):
        R.assert_amplification(amp, 'row at 20 std')
    with pytest.raises(AssertionError, match='amplification'):
        R.assert_amplification(R.fold_semantic(R.block(t), torch.zeros(M), M, R.block(k['wf']), k['c'], 1e-6)[4], 'row at 20 std')
    assert R.assert_amplification(R.fold_consumer(R.block(xhat), R.block(k['wf']), M, stats, k['colsum'], k['c'], 1e-6)[4], 'centred') < 1.1


def _kernel_like_attention_blk(qkv, B, N, H, scale, drop_last_key=False, sum_of_rounded=False):
    """attention_blk16.hip in fp32: exp2 of the scaled, max-subtracted scores, P -> bf16 for P.V (:209), the row sum of the UNROUNDED
    exponentials (:208) applied to the fp32 result (:276), one rounding at the store"""
    q, k, v = qkv.float().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * (scale / math.log(2))
    if drop_last_key:
        s[..., -1] = -math.inf
    e = torch.exp2(s - s.amax(-1, keepdim=True))
    eb = e.bfloat16().float()
    o = (eb @ v) / (eb if sum_of_rounded else e).sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(B * N, H * 64).bfloat16()


@pytest.mark.parametrize('N,amp', [(65, 1.5), (65, 4.0), (100, 4.0)])
def test_attention_blk_reference(N, amp):
    B, H = 2, 2
    g = _g(N)
    qkv = (torch.randn(B * N, 3 * H * 64, generator=g) * amp).bfloat16()
    qkv[:, 2 * H * 64:] += 0.75                                           # V with a non-zero mean: a dropped key does not average out
    r, m = R.attention_blk(R.block(qkv), B, N, H, 0.125)
    assert R.check(_kernel_like_attention_blk(qkv, B, N, H, 0.125), r, m, n_round=R.N_ROUND_ATT_BLK) <= 1.0
    if N == 65:
        assert R.check(_kernel_like_attention_blk(qkv, B, N, H, 0.125, drop_last_key=True), r, m, n_round=R.N_ROUND_ATT_BLK) > 1.0


def test_attention_blk_row_sum_of_the_rounded_probabilities_is_rejected():
    """The kernel normalises P.V by the sum of the UNROUNDED exponentials (attention_blk16.hip:208); the variant that sums the rounded ones
    errs by sum_j (p^_j - p_j) (v_j - o) instead of sum_j (p^_j - p_j) v_j.  On random inputs the two are alike, so the inputs are built to
    tell them apart: every query sees one key at the maximum (v = 0), 8 keys whose exponential 0.51375 rounds UP by 0.93 of the bf16 unit
    roundoff (v = a_d in [1, 2)) and 56 keys whose exponential 0.50975 rounds DOWN by 0.97 of it (v = 0) -- for the variant both groups push
    the result the same way, past what one counted rounding allows at some column a_d."""
    B, N, H, n_up = 1, 65, 2, 8
    qkv = torch.zeros(B * N, 3, H, 64)
    qkv[:, 0, :, 0], qkv[:, 0, :, 1] = 1.375, 1.5                          # s = 1.375 * -3.875 (up) | 1.5 * -3.59375 (down) | 0 (key 0)
    qkv[1:1 + n_up, 1, :, 0] = -3.875
    qkv[1 + n_up:, 1, :, 1] = -3.59375
    qkv[1:1 + n_up, 2] = 1.0 + torch.arange(128).float().view(H, 64) / 128.0
    qkv = qkv.reshape(B * N, 3 * H * 64).bfloat16()
    r, m = R.attention_blk(R.block(qkv), B, N, H, 0.125)
    good = R.check(_kernel_like_attention_blk(qkv, B, N, H, 0.125), r, m, n_round=R.N_ROUND_ATT_BLK)
    bad = R.check(_kernel_like_attention_blk(qkv, B, N, H, 0.125, sum_of_rounded=True), r, m, n_round=R.N_ROUND_ATT_BLK)
    assert good <= 1.0 < bad, (good, bad)


def test_layernorm_blk_and_patch_gather_references():
    g = _g(30)
    rows, C = 39, 256
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    for mean, std in ((0.5, 3.0), (40.0, 2.0)):
        x = torch.randn(rows, C, generator=g) * std + mean
        (r, m), (rm, mm) = R.layernorm_blk(R.block(x), rows, gam, bet, 1e-6)
        y = torch.nn.functional.layer_norm(x, (C,), gam, bet, 1e-6)
        assert R.check(y, r, m) <= 1.0 and R.check(y.bfloat16(), r, m) <= 1.0 and R.check(x.mean(1), rm, mm) <= 1.0
        assert R.check(x[:, :-1].sum(1) / C, rm, mm) > 1.0                                         # a mean without one column
        if mean < 10:
            assert R.check(torch.nn.functional.layer_norm(x, (C,), gam, bet, 1e-3), r, m) > 1.0      # another eps
    img = torch.randn(3, 3, 36, 20, generator=g)
    blk = R.patch_im2col_blk(img, 16, 2)
    assert blk.shape == (1, 96, 32, 8) and blk.dtype == torch.bfloat16
    assert torch.equal(R.unblock(blk, 6), R.patch_im2col(img, 16, 2, torch.bfloat16)) and not R.unblock(blk, 32)[6:].any()


@pytest.mark.parametrize('size,dim,heads', [((224, 224), 768, 12), ((256, 192), 768, 12), ((256, 192), 1024, 16)])
def test_fold_amplification_condition_holds_on_the_oracle_streams(size, dim, heads):
    """the condition the fold tests of the model configurations rest on (tests/test_vit_blocked_bf16_calls_gpu.py), from the CPU oracle at
    batch 2, depth 2: each residual stream minus its row means one residual step earlier has (E[x^2] + mean^2) / (var + eps) <= AMP_MAX"""
    from oracle import synth
    from oracle.vit import vit_tokens
    sd = synth.make_vit_state(21, size, embed_dim=dim, depth=2)
    x = synth.make_inputs(2, 22, size)['x']
    taps = {}
    vit_tokens(sd, x, num_heads=heads, taps=taps)
    st = [t.reshape(-1, dim).double() for t in taps['streams']]
    assert len(st) == 5
    worst = 0.0
    for prev, cur in zip(st[:-1], st[1:]):
        xs = cur - prev.mean(1, keepdim=True)
        _, _, amp = R._row_stats(xs.sum(1), (xs * xs).sum(1), dim, 1e-6)
        worst = max(worst, amp.max().item())
    print('fold amplification on the oracle streams %s dim %d: worst %.3f' % (size, dim, worst))
    assert worst <= R.AMP_MAX
