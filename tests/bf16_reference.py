"""Float64 references of the bf16 ViT training kernels, with error bounds derived from the kernels' own arithmetic.

A plain helper module (not collected by pytest); works on CPU and on device tensors.  Every reference takes the inputs of one library call
AS THE KERNEL RECEIVED THEM (bf16 or fp32 values) and returns ``(r, m)``:

  * ``r``: the exact result in float64;
  * ``m``: its magnitude -- the same expression with every operand replaced by its absolute value and every subtraction by an addition
    (``|A| . |B|^T`` for a GEMM, ``sum |dy * xhat|`` for dgamma).

``check`` then applies, element by element,

    |y - r| <= rho_out * |r| + (kappa_acc + n_round * 2^-8) * m + alpha

  * ``rho_out``: 2^-8 for a bf16 output (one round-to-nearest-even, with a spare ulp), 2^-22 for fp32;
  * ``kappa_acc`` <= 2^-15: fp32 accumulation and the other fp32 roundings on the way (2^-20 for the long column sums, KAPPA_SUM);
  * ``n_round``: the intermediate bf16 roundings the kernel does by design on the way to that output (counted next to each reference,
    with the kernel line that rounds);
  * ``alpha``: only the approximation errors that csrc/common.h documents (gelu_fast, gelu_grad_fast2).

Results that are a single rounding of something the kernel computed itself are compared bit for bit by the callers (``torch.equal``).
"""
import math

import torch

U8 = 2.0 ** -8                   # one bf16 rounding (RNE: half an ulp = 2^-9 relative, one spare)
RHO_BF16 = 2.0 ** -8
RHO_F32 = 2.0 ** -22
KAPPA = 2.0 ** -15
# the long fp32 column sums (TN weight gradients and their db, colsum, LayerNorm dgamma / dbeta: up to 12 544 rows).  Their worst case, n * 2^-24,
# would be vacuous; the error of such a sum of signed terms, relative to m, is of order 2^-24 (rounding errors of random sign), so 2^-20
# leaves a margin of 16 on that and is met with a margin of 3 or more at every shape the tests run.
KAPPA_SUM = 2.0 ** -20
GELU_ABS = 1.9e-4                # common.h: |gelu_fast - gelu_erf| <= 1.9e-4 absolute
GELU_GRAD_REL = 2.6e-4           # common.h: |gelu_grad_fast2 - gelu'| <= 2.6e-4 absolute, so the product errs by <= 2.6e-4 |a . w^T|
LN2 = math.log(2.0)

# intermediate bf16 roundings by design, per output (the kernel line that rounds)
N_ROUND_GEMM = 0                 # fp32 accumulate, one rounding at the store (counted by rho_out)
N_ROUND_GEMM_GELU_BWD = 1        # gemm_bf16_big_body.inc: the accumulator is staged as bf16 (LDS) before "* gelu'(z)" (pack_bf16x2 at :459)
N_ROUND_ATT_FWD = 1              # attention.hip:309: P -> bf16 for the P.V MFMA
N_ROUND_ATT_BWD_DV = 2           # attention.hip:446 dO -> bf16, :603 P -> bf16
N_ROUND_ATT_BWD_DQK = 2          # attention.hip:446 dO -> bf16 (dP = dO.V^T), :539 / :604 dS -> bf16


def _d(t):
    return None if t is None else t.detach().double()


def rho_of(t):
    return RHO_BF16 if t.dtype == torch.bfloat16 else RHO_F32


def check(y, r, m, n_round=0, alpha=0.0, kappa=KAPPA, rho_out=None):
    """worst ratio of |y - r| to its allowance over all elements (<= 1 passes); NaN / inf in y count as infinite error."""
    if rho_out is None:
        rho_out = rho_of(y)
    y = y.detach().double().reshape(r.shape)
    err = torch.nan_to_num((y - r).abs(), nan=math.inf, posinf=math.inf)
    allow = rho_out * r.abs() + (kappa + n_round * U8) * m + alpha
    ratio = torch.where(err == 0, torch.zeros_like(err), err / allow.clamp_min(1e-300))
    return ratio.max().item() if ratio.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------- forward


def patch_im2col(x, P, pad, dtype):
    """whmr_patch_im2col: the exact gather (rows (b, py, px), columns (c, ky, kx), zero padding), one cast -> compare bit for bit."""
    B = x.shape[0]
    cols = torch.nn.functional.unfold(x.float(), P, padding=pad, stride=P)            # [B, Cin P P, L]
    return cols.transpose(1, 2).reshape(B * cols.shape[2], cols.shape[1]).to(dtype)


def gemm(a, w, bias=None, residual=None, res_row_mod=0, row_scale=None):
    """out = residual + row_scale[m] * (a . w^T + bias)  (residual row m % res_row_mod when res_row_mod > 0)."""
    a, w = _d(a), _d(w)
    r, m = a @ w.t(), a.abs() @ w.abs().t()
    if bias is not None:
        r, m = r + _d(bias), m + _d(bias).abs()
    if row_scale is not None:
        rs = _d(row_scale).view(-1, 1)
        r, m = r * rs, m * rs.abs()
    if residual is not None:
        res = _d(residual).reshape(-1, r.shape[1])
        if res_row_mod > 0:
            res = res[torch.arange(r.shape[0], device=r.device) % res_row_mod]
        r, m = r + res, m + res.abs()
    return r, m


def gelu(z):
    """exact-erf GELU of the values given (fc1's pre-activation as the kernel stored it) -> r; the kernel's gelu_fast is within GELU_ABS."""
    z = _d(z)
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad(z):
    z = _d(z)
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def gemm_gelu_bwd(a, w, z):
    """fc2's data gradient times gelu'(z) (gemm gelu_bwd_of=z) -> (r, m, alpha); n_round = N_ROUND_GEMM_GELU_BWD."""
    lin, mlin = gemm(a, w)
    gg = gelu_grad(z)
    return lin * gg, mlin * gg.abs(), GELU_GRAD_REL * (lin.abs() + U8 * mlin)


def layernorm(x, gamma, beta, eps):
    """y = (x - mean) * rstd * gamma + beta;  m = (|x| + |mean|) * rstd * |gamma| + |beta|."""
    x, g, b = _d(x), _d(gamma), _d(beta)
    mu = x.mean(-1, keepdim=True)
    rstd = ((x - mu).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    return (x - mu) * rstd * g + b, (x.abs() + mu.abs()) * rstd * g.abs() + b.abs()


def attention_fwd(qkv, B, N, H, d, scale, chunk=96):
    """softmax(q k^T scale) v per (image, head) from qkv [B*N, 3*H*d] -> ((o, m_o), (lse, m_lse)).
    o: [B*N, H*d], m_o = P . |v| (P >= 0), n_round = N_ROUND_ATT_FWD.  lse: [B*H*N] in the log2 domain the kernel works in
    (logsumexp / ln 2); m_lse = max_j |q||k|_j scale / ln 2 + 1 (the fp32 logits and the fp32 log2 of the row sum)."""
    q, k, v = _d(qkv).view(B, N, 3, H, d).permute(2, 0, 3, 1, 4).reshape(3, B * H, N, d)
    o, mo = torch.empty_like(q), torch.empty_like(q)
    lse, ml = torch.empty(B * H, N, dtype=torch.float64, device=q.device), torch.empty(B * H, N, dtype=torch.float64, device=q.device)
    for i in range(0, B * H, chunk):
        sl = slice(i, i + chunk)
        s = (q[sl] @ k[sl].transpose(-1, -2)) * scale
        p = torch.softmax(s, -1)
        o[sl], mo[sl] = p @ v[sl], p @ v[sl].abs()
        lse[sl] = torch.logsumexp(s, -1) / LN2
        ml[sl] = ((q[sl].abs() @ k[sl].abs().transpose(-1, -2)) * scale).amax(-1) / LN2 + 1.0
    back = lambda t: t.view(B, H, N, d).permute(0, 2, 1, 3).reshape(B * N, H * d)
    return (back(o), back(mo)), (lse.reshape(-1), ml.reshape(-1))


def attention_bwd(qkv, o, dout, lse, B, N, H, d, scale, chunk=96):
    """whmr_attention_bwd with the lse it was GIVEN (an input of the call): P = exp2(s log2e - lse), D = rowsum(dO o),
    dS = P (dO.V^T - D), dQ = scale dS.K, dK = scale dS^T.Q, dV = P^T.dO  ->  (r, m) of dqkv [B*N, 3*H*d].
    n_round: dQ / dK N_ROUND_ATT_BWD_DQK, dV N_ROUND_ATT_BWD_DV."""
    q, k, v = _d(qkv).view(B, N, 3, H, d).permute(2, 0, 3, 1, 4).reshape(3, B * H, N, d)
    ob = _d(o).view(B, N, H, d).permute(0, 2, 1, 3).reshape(B * H, N, d)
    dob = _d(dout).view(B, N, H, d).permute(0, 2, 1, 3).reshape(B * H, N, d)
    ls = _d(lse).view(B * H, N, 1)
    r, m = torch.empty(3, B * H, N, d, dtype=torch.float64, device=q.device), torch.empty(3, B * H, N, d, dtype=torch.float64, device=q.device)
    for i in range(0, B * H, chunk):
        sl = slice(i, i + chunk)
        p = torch.exp((q[sl] @ k[sl].transpose(-1, -2)) * scale - ls[sl] * LN2)
        D, mD = (dob[sl] * ob[sl]).sum(-1, keepdim=True), (dob[sl] * ob[sl]).abs().sum(-1, keepdim=True)
        dp, mdp = dob[sl] @ v[sl].transpose(-1, -2), dob[sl].abs() @ v[sl].abs().transpose(-1, -2)
        ds, mds = p * (dp - D), p * (mdp + mD)
        r[0, sl], m[0, sl] = scale * (ds @ k[sl]), scale * (mds @ k[sl].abs())
        r[1, sl], m[1, sl] = scale * (ds.transpose(-1, -2) @ q[sl]), scale * (mds.transpose(-1, -2) @ q[sl].abs())
        r[2, sl], m[2, sl] = p.transpose(-1, -2) @ dob[sl], p.transpose(-1, -2) @ dob[sl].abs()
    back = lambda t: t.view(3, B, H, N, d).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * d)
    return back(r), back(m)


def attention_bwd_n_round(B, N, H, d, device):
    """per-element n_round of dqkv [B*N, 3*H*d]: the dQ / dK and dV column blocks"""
    nr = torch.tensor([N_ROUND_ATT_BWD_DQK, N_ROUND_ATT_BWD_DQK, N_ROUND_ATT_BWD_DV], dtype=torch.float64, device=device)
    return nr.view(1, 3, 1, 1).expand(B * N, 3, H, d).reshape(B * N, 3 * H * d)


# ---------------------------------------------------------------------------------------------------------------------------- backward


def layernorm_bwd(x, dy, gamma, eps, dres=None, dgamma_prior=None, dbeta_prior=None):
    """whmr_layernorm_bwd: dx = rstd (g - mean g - xhat mean(g xhat)) (+ dres), g = dy gamma; dgamma = sum dy xhat, dbeta = sum dy
    (+ the prior values when accumulating) -> {'dx': (r, m), 'dgamma': (r, m), 'dbeta': (r, m)}.  n_round 0 (all fp32); dgamma / dbeta
    are column sums over the rows: kappa KAPPA_SUM."""
    x, dy, g = _d(x), _d(dy), _d(gamma)
    mu = x.mean(-1, keepdim=True)
    rstd = ((x - mu).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xh, mxh = (x - mu) * rstd, (x.abs() + mu.abs()) * rstd
    gg, mg = dy * g, (dy * g).abs()
    dx = rstd * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    mdx = rstd * (mg + mg.mean(-1, keepdim=True) + mxh * (mg * mxh).mean(-1, keepdim=True))
    if dres is not None:
        dx, mdx = dx + _d(dres), mdx + _d(dres).abs()
    dgm, mdgm = (dy * xh).sum(0), (dy.abs() * mxh).sum(0)
    dbt, mdbt = dy.sum(0), dy.abs().sum(0)
    if dgamma_prior is not None:
        dgm, mdgm = dgm + _d(dgamma_prior), mdgm + _d(dgamma_prior).abs()
        dbt, mdbt = dbt + _d(dbeta_prior), mdbt + _d(dbeta_prior).abs()
    return {'dx': (dx, mdx), 'dgamma': (dgm, mdgm), 'dbeta': (dbt, mdbt)}


def cast_rows(dx, row_scale=None):
    """layernorm_bwd's cast_out: bf16(dx * row_scale[row]) of the kernel's own fp32 dx (one fp32 product, one RNE) -> bit for bit."""
    dx = dx.detach().float()
    if row_scale is not None:
        dx = dx * row_scale.detach().float().view(-1, 1)
    return dx.to(torch.bfloat16)


def gemm_tn(a, b, db=False):
    """whmr_gemm_tn_bf16: out = a^T . b for a [K, Mo], b [K, No] (+ db = column sums of a) -> (r, m) or ((r, m), (r_db, m_db)); kappa KAPPA_SUM."""
    a, b = _d(a), _d(b)
    out = (a.t() @ b, a.abs().t() @ b.abs())
    if not db:
        return out
    return out, (a.sum(0), a.abs().sum(0))


def colsum(x, prior=None):
    """whmr_colsum: out[c] = sum_r x[r, c] (+ prior); kappa KAPPA_SUM"""
    x = _d(x)
    r, m = x.sum(0), x.abs().sum(0)
    if prior is not None:
        r, m = r + _d(prior), m + _d(prior).abs()
    return r, m
