"""Float64 references of the bf16 ViT training kernels and of the blocked bf16 inference kernels, with error bounds derived from the kernels' own
arithmetic.

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


# ------------------------------------------------------------------------------------------- blocked bf16 inference path (csrc/gemm_blk16_impl.h,
# attention_blk16.hip, vit_ops.hip).  Operands arrive in the blocked layout [rows/32][cols/E][32][E] (E = 8 bf16 / 4 fp32) and are compared
# row-major; rows >= M of the last 32-row block are not part of any comparison.

EPI_BF16, EPI_BF16_GELU, EPI_F32_RES, EPI_F32_POS = 0, 1, 2, 3
N_ROUND_GEMM_BLK = 0             # gemm_blk16_impl.h:253-256 / :327-329: fp32 accumulator + bias (+ residual), one rounding at the store (rho_out)
N_ROUND_GEMM_BLK_GELU = 0        # gemm_blk16_impl.h:255: gelu_fast2 of the fp32 value in registers, rounded once at :256 (rho_out)
N_ROUND_FOLD_CONSUMER = 0        # gemm_blk16_impl.h:253-254: rstd * acc - rstd * mean * colsum + bias in fp32 fmas on the operand it was GIVEN
N_ROUND_FOLD_SEMANTIC = 1        # gemm_blk16_impl.h:338: the producer rounds the centred row to bf16 (xhat); carried as 2^-8 rstd |t - s| . |W'|^T
N_ROUND_ATT_BLK = 1              # attention_blk16.hip:209-210: P -> bf16 for the P.V MFMA; the row sum (:208, :258-265) is of the UNROUNDED
#                                  exponentials and scales the fp32 result (:276).  The N > 240 fallback does the same: attention.hip:309 / :293-296
GELU_LIP = 1.13                  # max |gelu'| = 1.1289: an error e of the pre-activation moves the exact GELU by at most 1.13 e
AMP_MAX = 4.0                    # every fold test asserts the amplification of its own inputs (below) is <= this


def unblock(t, rows):
    """blocked [rows/32][cols/E][32][E] -> row-major [rows, cols]"""
    nb, nu, _, E = t.shape
    return t.permute(0, 2, 1, 3).reshape(nb * 32, nu * E)[:rows]


def block(t):
    """row-major [R, C] -> blocked [ceil(R/32)][C/E][32][E], padding rows zero"""
    E = 8 if t.dtype == torch.bfloat16 else 4
    t = torch.cat([t, t.new_zeros(-t.shape[0] % 32, t.shape[1])], 0)
    return t.reshape(t.shape[0] // 32, 32, t.shape[1] // E, E).permute(0, 2, 1, 3).contiguous()


def _gelu_of(r, m, alpha=0.0):
    """the exact GELU of a pre-activation known to (r, m, alpha): gelu_fast2 is within GELU_ABS, and |gelu'| <= GELU_LIP"""
    return gelu(r), GELU_LIP * m, GELU_LIP * alpha + GELU_ABS


def gemm_blk(a, w, M, bias=None, epi=EPI_BF16, res=None, res_rows=0):
    """whmr_gemm_blk without the LayerNorm fold: a [M/32][K/8][32][8], w [N/32][K/8][32][8] bf16 -> (r, m, alpha) of the M x N result.
    EPI_BF16: a.w^T + bias;  EPI_BF16_GELU: its GELU (alpha GELU_ABS);  EPI_F32_RES: + the blocked fp32 residual as it was BEFORE the call
    (the kernel may run in place);  EPI_F32_POS: + res[m % res_rows] of a row-major fp32 table.  n_round 0 for all four."""
    A, W = unblock(a, M), unblock(w, w.shape[0] * 32)
    if epi == EPI_F32_RES:
        r, m = gemm(A, W, bias=bias, residual=unblock(res, M))
    elif epi == EPI_F32_POS:
        r, m = gemm(A, W, bias=bias, residual=res.reshape(-1, W.shape[0]), res_row_mod=res_rows)
    else:
        r, m = gemm(A, W, bias=bias)
    if epi == EPI_BF16_GELU:
        return _gelu_of(r, m)
    return r, m, 0.0


def fold_producer(C, M, shift=None, shift_stats=None, shift_out=None):
    """The emission of a folding producer (gemm_blk16_impl.h:276-299, 330-371), from the fp32 stream C it STORED (blocked, live) and its shift
    inputs as it received them ->
      s:      (r, m) of s_m = shift[m] + sum_t shift_stats[m, t, 0] / N in float64 (None without a shift) -- shift_out is held to it, fp32 bound;
      s_live: the fp32 shift the kernel applied (shift_out where it wrote one; a lone ``shift`` is applied as it is, :289);
      xhat:   bf16(fp32(C - s_live)), row-major [M, N]: ONE rounding (:338) of values the kernel computed itself -> compare bit for bit;
      stats:  (r, m) [M, N/256, 2] of (sum o, sum o^2) over the 256 columns of tile t, o = fp32(C - s_live) (:332-337, :359-369);
              magnitudes sum |o| and sum o^2, kappa KAPPA (a 256-term fp32 sum in a fixed tree)."""
    c = unblock(C, M).float()
    N = c.shape[1]
    T = N // 256
    s, s_live = None, torch.zeros(M, dtype=torch.float32, device=c.device)
    if shift is not None or shift_stats is not None:
        sr, sm = torch.zeros(M, dtype=torch.float64, device=c.device), torch.zeros(M, dtype=torch.float64, device=c.device)
        if shift is not None:
            sr, sm = sr + _d(shift).reshape(-1)[:M], sm + _d(shift).reshape(-1)[:M].abs()
        if shift_stats is not None:
            assert shift_out is not None, 'the applied shift is only known from shift_out'
            part = _d(shift_stats).reshape(-1, T, 2)[:M, :, 0]
            sr, sm = sr + part.sum(1) / N, sm + part.abs().sum(1) / N
        s = (sr, sm)
        s_live = (shift_out if shift_out is not None else shift).detach().float().reshape(-1)[:M]
    o = c - s_live.view(-1, 1)                                                      # fp32, as :332
    od = o.double().view(M, T, 256)
    sq = (od * od).sum(-1)
    stats = (torch.stack([od.sum(-1), sq], -1), torch.stack([od.abs().sum(-1), sq], -1))
    return {'s': s, 's_live': s_live, 'xhat': o.to(torch.bfloat16), 'stats': stats}


def _row_stats(sx, sxx, K, eps):
    """mean, rstd and the amplification (E[x^2] + mean^2) / (var + eps) of rows known by their sums.

    The consumer forms var = E2 - mean^2 (E2 = sum sxx / K) in one pass in fp32 (gemm_blk16_impl.h:226-229).  E2 and mean^2 each carry a
    relative error <= kappa, so |d var| <= kappa (E2 + mean^2); rstd = (var + eps)^-1/2 gives d rstd / rstd = -1/2 d var / (var + eps), i.e.
    |d rstd| / rstd <= 1/2 kappa (E2 + mean^2) / (var + eps) = 1/2 kappa amp.  Every term of the result but the bias is proportional to rstd,
    so the allowance of a consumer is kappa (1 + amp / 2) m.  amp is 1 + 2 mean^2 / var: 1 for a centred row, 801 at |mean| = 20 std --
    which is why the tests ASSERT amp <= AMP_MAX on their inputs instead of letting the bound grow with it."""
    mean = sx / K
    e2 = sxx / K
    var = (e2 - mean * mean).clamp_min(0.0)
    return mean, (var + eps).rsqrt(), (e2 + mean * mean) / (var + eps)


def assert_amplification(amp, what):
    """the CONDITION of every fold check: the rows' amplification is <= AMP_MAX (so kappa (1 + amp / 2) <= 3 kappa) -> the worst one"""
    a = amp.max().item()
    assert a <= AMP_MAX, '%s: amplification %.3g of the row statistics exceeds %g -- these inputs do not meet the fold checks\' condition' % (what, a, AMP_MAX)
    return a


def fold_consumer(a, w, M, stats_in, colsum, bias, eps, epi=EPI_BF16):
    """A fold consumer (gemm_blk16_impl.h:212-261) from the operands it was given: a = the producer's bf16 copy, w = W' = bf16(gamma o W),
    stats_in [rows][K/256][2], colsum, bias = c -> (r, m, kappa [M, 1], alpha, amp [M]):
        mean = sum_t sx / K,  var = max(sum_t sxx / K - mean^2, 0),  rstd = (var + eps)^-1/2
        r = rstd (a . W'^T) - rstd mean colsum + bias,   m = rstd (|a| . |W'|^T + |mean| |colsum|) + |bias|
    kappa = KAPPA (1 + amp / 2) per row (``_row_stats``).  EPI_BF16_GELU: the GELU of that."""
    A, W = unblock(a, M), unblock(w, w.shape[0] * 32)
    K = A.shape[1]
    st = _d(stats_in).reshape(-1, K // 256, 2)[:M]
    mean, rstd, amp = _row_stats(st[..., 0].sum(1), st[..., 1].sum(1), K, eps)
    lin, mlin = gemm(A, W)
    cs = _d(colsum).view(1, -1)
    b = _d(bias).view(1, -1) if bias is not None else torch.zeros_like(cs)
    mean, rstd = mean.view(-1, 1), rstd.view(-1, 1)
    r = rstd * lin - rstd * mean * cs + b
    m = rstd * (mlin + mean.abs() * cs.abs()) + b.abs()
    kappa = KAPPA * (1.0 + 0.5 * amp).view(-1, 1)
    if epi == EPI_BF16_GELU:
        return _gelu_of(r, m) + (kappa, amp)
    return r, m, 0.0, kappa, amp


def fold_colsum(w):
    """colsum[n] = sum_k W'[n, k] of the ROUNDED operand the MFMAs multiply (only then does the mean term cancel) -> (r, m); a long fp32 sum
    made on the host side: kappa KAPPA_SUM"""
    W = _d(unblock(w, w.shape[0] * 32))
    return W.sum(1), W.abs().sum(1)


def fold_semantic(C, s, M, w, bias, eps, epi=EPI_BF16):
    """What a fold consumer's output MEANS: LN(t) . W^T as rstd ((t - s) - mean) . W'^T + c, in float64 from the fp32 stream t = C the producer
    left (blocked, live), the shift s it applied, and W', c as the consumer got them; mean and rstd are the TRUE statistics of t - s.
    -> (r, m, alpha, kappa [M, 1], amp [M]):  m = rstd ((|t - s| + |mean|) . |W'|^T) + |c|;  alpha = 2^-8 rstd |t - s| . |W'|^T, the one bf16
    rounding of the centred row (N_ROUND_FOLD_SEMANTIC).  A consumer that reads another step's statistics, or a producer whose sums and
    copy disagree, is correct call by call and fails here."""
    x = unblock(C, M).double() - s.detach().double().reshape(-1)[:M].view(-1, 1)
    W = _d(unblock(w, w.shape[0] * 32))
    K = x.shape[1]
    mean, rstd, amp = _row_stats(x.sum(1), (x * x).sum(1), K, eps)
    mean, rstd = mean.view(-1, 1), rstd.view(-1, 1)
    b = _d(bias).view(1, -1) if bias is not None else 0.0
    mx = x.abs() @ W.abs().t()
    r = rstd * ((x - mean) @ W.t()) + b
    m = rstd * (mx + mean.abs() * W.abs().sum(1).view(1, -1)) + (b.abs() if bias is not None else 0.0)
    alpha = N_ROUND_FOLD_SEMANTIC * U8 * rstd * mx
    kappa = KAPPA * (1.0 + 0.5 * amp).view(-1, 1)
    if epi == EPI_BF16_GELU:
        return _gelu_of(r, m, alpha) + (kappa, amp)
    return r, m, alpha, kappa, amp


def attention_blk(qkv, B, N, H, scale, chunk=96):
    """whmr_attention_blk (d = 64): ``attention_fwd`` on the unblocked qkv -> (r, m) of o [B*N, H*64]; n_round N_ROUND_ATT_BLK"""
    return attention_fwd(unblock(qkv, B * N), B, N, H, 64, scale, chunk)[0]


def layernorm_blk(x, rows, gamma, beta, eps):
    """whmr_layernorm_blk on the blocked fp32 stream -> ((r, m) of the result [rows, C], (r, m) of the row means).  Two-pass statistics in fp32
    (vit_ops.hip:205-229), n_round 0: the bf16 operand form rounds once at the store (rho_out), out_std and mean_out are fp32."""
    xr = unblock(x, rows)
    xd = _d(xr)
    return layernorm(xr, gamma, beta, eps), (xd.mean(1), xd.abs().mean(1))


def patch_im2col_blk(x, P, pad):
    """whmr_patch_im2col_blk: the exact gather of ``patch_im2col`` in the blocked layout, padding rows zero -> compare bit for bit"""
    return block(patch_im2col(x, P, pad, torch.bfloat16))
