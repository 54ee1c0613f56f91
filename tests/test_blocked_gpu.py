"""Blocked-layout kernels of the bf16 ViT inference path (csrc/gemm_blk.hip + blocked LayerNorm / attention / patch gather) against
plain fp32 torch on the same inputs, and the blocked ViT forward against the row-major path and the reference fixture."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TILES = [0x44, 0x55, 0x43, 0x33, 0x32, 0x22, 0x54, 0x21]


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def test_blocked_layout_round_trip(dev):
    from whmr_amd import _lib as L
    g = torch.Generator().manual_seed(0)
    for dt, E in ((torch.bfloat16, 8), (torch.float32, 4)):
        x = torch.randn(70, 64, generator=g).to(dt).to(dev)
        xb = L.to_blocked(x)
        assert xb.shape == (3, 64 // E, 32, E)
        assert torch.equal(L.from_blocked(xb, 70), x)
        # element (r, c) sits at [r // 32][c // E][r % 32][c % E]
        assert xb[1, 3, 5, 2] == x[37, 3 * E + 2]


@pytest.mark.parametrize('M,N,K', [(392, 768, 768), (1000, 256, 32), (1001, 512, 64), (777, 256, 96), (12544, 2304, 768), (3000, 768, 3072)])
@pytest.mark.parametrize('tile', [0] + TILES)
def test_gemm_blk(dev, M, N, K, tile):
    """every epilogue x every tile: asymmetric random operands (a transposed C write cannot pass), M tails that end inside a tile and inside
    a 32-row block, K of 1 / 2 / 3 half tiles (ring prologue edge cases) up to the ViT shapes"""
    from whmr_amd import _lib as L
    if M > 4000 and tile not in (0, 0x44, 0x43, 0x55):
        pytest.skip('full-size shape: chooser + the tiles the ViT uses')
    g = torch.Generator().manual_seed(M + N + K + tile)
    a = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16()
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    pos = torch.randn(196, N, generator=g)
    ab, wb = L.to_blocked(a.to(dev)), L.to_blocked(w.to(dev))
    nb = ab.shape[0]
    lin = a.float() @ w.float().t() + bias
    # epi 0: bf16(acc + bias)
    out = torch.full((nb, N // 8, 32, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    L.gemm_blk(ab, wb, out, M, bias=bias.to(dev), epi=L.EPI_BF16, tile=tile)
    assert _rel(L.from_blocked(out, M).float().cpu(), lin) < 1e-2
    # no bias
    L.gemm_blk(ab, wb, out, M, epi=L.EPI_BF16, tile=tile)
    assert _rel(L.from_blocked(out, M).float().cpu(), a.float() @ w.float().t()) < 1e-2
    # epi 1: bf16(gelu(acc + bias))  (polynomial GELU: <= 1.9e-4 absolute from the erf form)
    L.gemm_blk(ab, wb, out, M, bias=bias.to(dev), epi=L.EPI_BF16_GELU, tile=tile)
    assert _rel(L.from_blocked(out, M).float().cpu(), F.gelu(lin)) < 1e-2
    # epi 2: fp32 acc + bias + blocked residual, in place
    t = L.to_blocked(res.to(dev))
    L.gemm_blk(ab, wb, t, M, bias=bias.to(dev), epi=L.EPI_F32_RES, res=t, tile=tile)
    assert _rel(L.from_blocked(t, M).cpu(), lin + res) < 2e-5 * math.sqrt(K) / 8 + 1e-5
    # epi 3: fp32 acc + bias + pos[m % 196] (row-major residual)
    t2 = torch.full((nb, N // 4, 32, 4), float('nan'), device=dev)
    L.gemm_blk(ab, wb, t2, M, bias=bias.to(dev), epi=L.EPI_F32_POS, res=pos.to(dev), res_rows=196, tile=tile)
    assert _rel(L.from_blocked(t2, M).cpu(), lin + pos[torch.arange(M) % 196]) < 2e-5 * math.sqrt(K) / 8 + 1e-5


def test_gemm_blk_matches_row_major_kernel_bitwise(dev):
    """same MFMA instruction, same k order: the blocked kernel and the row-major kernel must agree bit for bit on an exact epilogue"""
    from whmr_amd import _lib as L
    g = torch.Generator().manual_seed(5)
    M, N, K = 1568, 768, 768
    a = torch.randn(M, K, generator=g).bfloat16().to(dev)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    res = torch.randn(M, N, generator=g).to(dev)
    ref = torch.empty(M, N, device=dev)
    L.gemm(a, w, ref, bias=bias, residual=res)
    t = L.to_blocked(res)
    L.gemm_blk(L.to_blocked(a), L.to_blocked(w), t, M, bias=bias, epi=L.EPI_F32_RES, res=t)
    assert torch.equal(L.from_blocked(t, M), ref)



@pytest.mark.parametrize('C', [768, 1024, 256])
def test_layernorm_blk(dev, C):
    """whmr_layernorm_blk (vit.py:125,133,242 on the blocked stream; models/pose_vit.py uses it for the unfolded LayerNorms and the final norm):
    blocked bf16 operand form and row-major fp32 form against F.layer_norm and the row-major kernel; ragged last row block (391 rows)"""
    from whmr_amd import _lib as L
    g = torch.Generator().manual_seed(C)
    rows = 391
    x = torch.randn(rows, C, generator=g) * 3 + 0.5
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.layer_norm(x, (C,), w, b, 1e-6)
    xb = L.to_blocked(x.to(dev))
    out = torch.empty(xb.shape[0], C // 8, 32, 8, device=dev, dtype=torch.bfloat16)
    L.layernorm_blk(xb, w.to(dev), b.to(dev), out, rows, 1e-6)
    assert _rel(L.from_blocked(out, rows).float().cpu(), ref) < 1e-2
    std = torch.empty(rows, C, device=dev)
    L.layernorm_blk(xb, w.to(dev), b.to(dev), std, rows, 1e-6, out_std=True)
    assert _rel(std.cpu(), ref) < 2e-6
    # against the row-major kernel: same two-pass statistics, different summation tree -> fp32 rounding only
    rm = torch.empty(rows, C, device=dev)
    L.layernorm(x.to(dev), w.to(dev), b.to(dev), rm, 1e-6)
    assert _rel(std, rm) < 2e-6


@pytest.mark.parametrize('N,B', [(196, 3), (192, 3), (100, 3), (256, 3), (65, 2), (208, 2), (196, 64), (192, 27)])
def test_attention_blk(dev, N, B):
    """whmr_attention_blk (round 5: the persistent 16-row-tile kernel, csrc/attention_blk16.hip) against fp32 torch on the same bf16 inputs, and
    against the round-2 blocked kernel (variant bit 4).  B = 64 / 27: 768 / 324 (image, head) items on 256 workgroups -- three / one-or-two
    items per workgroup, i.e. the double-buffered LDS halves and the prefetch of the next item's K / V / Q are exercised; N = 65 / 208 / 256:
    one real row in the last query tile / an exact tile multiple / 16 waves."""
    from whmr_amd import _lib as L
    g = torch.Generator().manual_seed(N)
    H, d = 12, 64
    qkv = (torch.randn(B, N, 3, H, d, generator=g) * 1.5).bfloat16()
    q, k, v = qkv.float().permute(2, 0, 3, 1, 4)
    ref = ((q * d ** -0.5) @ k.transpose(-2, -1)).softmax(-1) @ v
    ref = ref.transpose(1, 2).reshape(B * N, H * d)
    qb = L.to_blocked(qkv.view(B * N, 3 * H * d).to(dev))
    out = torch.full((qb.shape[0], H * d // 8, 32, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    L.attention_blk(qb, out, B, N, H, d ** -0.5)
    got = L.from_blocked(out, B * N)
    assert torch.isfinite(got.float()).all()
    # bf16 P and bf16 output: per element within 1.5 bf16 ulps of the row's scale (measured ~4e-3 max-rel)
    assert _rel(got.float().cpu(), ref) < 1e-2
    assert ((got.float().cpu() - ref).abs().max(1).values / ref.abs().max(1).values).max() < 2e-2          # every ROW (token), not only the largest
    # padding rows of the last 32-row block are not written
    if (B * N) % 32:
        assert torch.isnan(L.from_blocked(out, qb.shape[0] * 32)[B * N:].float()).all()
    # the round-2 kernel (online softmax over 64-key chunks, 32-row tiles) on the same operands: same arithmetic up to the softmax's summation order
    old = torch.full_like(out, float('nan'))
    L.attention_set_variant(1 | 16)
    try:
        L.attention_blk(qb, old, B, N, H, d ** -0.5)
    finally:
        L.attention_set_variant(1)
    assert _rel(got.float(), L.from_blocked(old, B * N).float()) < 1e-2
    # deterministic
    again = torch.full_like(out, float('nan'))
    L.attention_blk(qb, again, B, N, H, d ** -0.5)
    assert torch.equal(L.from_blocked(again, B * N), got)


def test_patch_im2col_blk(dev):
    from whmr_amd import _lib as L
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 3, 64, 80, generator=g)[:, :, :, 8:-8]             # sliced view like demo/tester.py:152
    M = 3 * 4 * 4                                                        # 48 rows: the second 32-row block is half padding
    out = torch.full(((M + 31) // 32, 768 // 8, 32, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    L.patch_im2col_blk(x.to(dev)[:, :, :, :], out, 16, 2)
    ref = F.unfold(x, 16, padding=2, stride=16).transpose(1, 2).reshape(-1, 768).bfloat16()
    assert torch.equal(L.from_blocked(out, M).cpu(), ref)
    assert torch.equal(L.from_blocked(out, 64)[M:].cpu(), torch.zeros(64 - M, 768, dtype=torch.bfloat16))   # padding rows are zero, not garbage


def _vit(sd, size, dev, blocked, dim=768, depth=12, heads=12):
    from whmr_amd.models.pose_vit import ViT
    m = ViT(img_size=size, patch_size=16, embed_dim=dim, depth=depth, num_heads=heads, ratio=1, mlp_ratio=4, qkv_bias=True, numerics='bf16')
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    m.blocked = blocked
    m.blocked_min_tokens = 0              # these tests exercise the blocked path at small batch (the product switches to it from ~2k tokens)
    return m


def test_vit_blocked_path_matches_row_major_path_and_fixture(dev):
    """ViT-B/16 224^2 (BASELINE configs[1]) in bf16: the blocked pipeline against the row-major kernels (same arithmetic up to the fp32
    summation order of LayerNorm) and against the reference fixture (fp32 CPU forward of the imported reference)."""
    from oracle import synth
    g = np.load(os.path.join(GOLDEN, 'vit224_b2.npz'))
    sd = synth.make_vit_state(1, (224, 224))
    x = torch.from_numpy(g['x']).to(dev)
    ref = torch.from_numpy(g['s_feat'])
    out_b = _vit(sd, (224, 224), dev, True)(x)
    out_r = _vit(sd, (224, 224), dev, False)(x)
    assert out_b.shape == (2, 768, 14, 14)
    eb, er = _rel(out_b.cpu(), ref), _rel(out_r.cpu(), ref)
    print('bf16 ViT vs fp32 reference fixture: blocked %.3e, row-major %.3e, blocked vs row-major %.3e' % (eb, er, _rel(out_b, out_r)))
    assert eb < 5e-2 and er < 5e-2
    assert _rel(out_b, out_r) < 2e-2


def test_vit_blocked_256x192_and_large(dev):
    """the other backbone shapes on the blocked path: 256x192 (N = 192 tokens, ref-native) and ViT-L (dim 1024, 16 heads, depth 2) vs the CPU oracle"""
    from oracle import synth
    from oracle.vit import vit_forward
    for dim, depth, heads in ((768, 2, 12), (1024, 2, 16)):
        sd = synth.make_vit_state(3, (256, 192), embed_dim=dim, depth=depth)
        x = synth.make_inputs(3, 9, (256, 192))['x']
        ref = vit_forward(sd, x, num_heads=heads)
        out = _vit(sd, (256, 192), dev, True, dim, depth, heads)(x.to(dev))
        assert out.shape == (3, dim, 16, 12)
        assert _rel(out.cpu(), ref) < 5e-2, dim


def test_vit_blocked_full_size_properties(dev):
    """BASELINE batch-64 size: per-image independence on the blocked path, bit for bit (a batch of 64 == the same images in two halves;
    the tile chooser picks different tile heights for M = 12544 and M = 6272) and the result is a fresh tensor per call"""
    from oracle import synth
    sd = synth.make_vit_state(1, (224, 224))
    m = _vit(sd, (224, 224), dev, True)
    x = synth.make_inputs(64, 3, (224, 224))['x'].to(dev)
    full = m(x)
    a = m(x[:32])
    b = m(x[32:])
    assert torch.equal(full, torch.cat([a, b]))
    assert torch.isfinite(full).all()
    assert full.data_ptr() != a.data_ptr() and a.data_ptr() != b.data_ptr()


@pytest.mark.parametrize('tile', [0, 0x44, 0x32, 0x55])
def test_gemm_blk_layernorm_fold(dev, tile):
    """LayerNorm folded into the GEMM pair (vit.py:125-126,133-134): the producer (epi 2) also emits bf16(stream) + per-row partial sums, the
    consumer (epi 0 / 1) multiplies the raw copy by gamma-scaled weights and normalises in its epilogue -- against LayerNorm + Linear in fp32 torch"""
    from whmr_amd import _lib as L
    g = torch.Generator().manual_seed(9 + tile)
    M, C, N2 = 1000, 768, 2304
    att = torch.randn(M, C, generator=g).bfloat16()
    wp = (torch.randn(C, C, generator=g) / math.sqrt(C)).bfloat16()
    bp = torch.randn(C, generator=g)
    t0 = torch.randn(M, C, generator=g) * 2 + 0.7                       # residual stream with a non-zero mean
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1, torch.randn(C, generator=g) * 0.2
    w2 = torch.randn(N2, C, generator=g) / math.sqrt(C)
    b2 = torch.randn(N2, generator=g)
    # reference: t1 = t0 + att.wp^T + bp ; out = LN(t1).w2^T + b2
    t1 = t0 + att.float() @ wp.float().t() + bp
    ref = F.layer_norm(t1, (C,), gamma, beta, 1e-6) @ w2.t() + b2
    tb = L.to_blocked(t0.to(dev))
    nb = tb.shape[0]
    xhat = torch.full((nb, C // 8, 32, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    stats = torch.full((nb * 32, C // 256, 2), float('nan'), device=dev)
    L.gemm_blk(L.to_blocked(att.to(dev)), L.to_blocked(wp.to(dev)), tb, M, bias=bp.to(dev), epi=L.EPI_F32_RES, res=tb, tile=tile, xhat=xhat, stats_out=stats)
    got_t1 = L.from_blocked(tb, M).cpu()
    assert _rel(got_t1, t1) < 1e-5
    assert torch.equal(L.from_blocked(xhat, M).cpu(), got_t1.bfloat16())                      # the emitted operand is exactly bf16(stream)
    st = stats[:M].cpu().double().sum(1)
    assert _rel(st[:, 0], got_t1.double().sum(1)) < 1e-5 and _rel(st[:, 1], (got_t1.double() ** 2).sum(1)) < 1e-5
    wf = (w2 * gamma[None, :]).bfloat16()
    s = wf.float().sum(1)
    c = b2 + w2 @ beta
    out = torch.full((nb, N2 // 8, 32, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    L.gemm_blk(xhat, L.to_blocked(wf.to(dev)), out, M, bias=c.to(dev), epi=L.EPI_BF16, tile=tile, stats_in=stats, colsum=s.to(dev), ln_eps=1e-6)
    err = _rel(L.from_blocked(out, M).float().cpu(), ref)
    # same error class as the unfolded bf16 path: LayerNorm output rounded to bf16, then a bf16 GEMM
    h_ref = F.layer_norm(t1, (C,), gamma, beta, 1e-6).bfloat16().float() @ w2.bfloat16().float().t() + b2
    print('folded LayerNorm + qkv: max-rel %.2e (unfolded bf16 pipeline: %.2e)' % (err, _rel(h_ref, ref)))
    assert err < 1.5e-2
    L.gemm_blk(xhat, L.to_blocked(wf.to(dev)), out, M, bias=c.to(dev), epi=L.EPI_BF16_GELU, tile=tile, stats_in=stats, colsum=s.to(dev), ln_eps=1e-6)
    assert _rel(L.from_blocked(out, M).float().cpu(), F.gelu(ref)) < 1.5e-2


def test_vit_ln_fold_matches_unfolded(dev):
    """ViT-B 224^2 bf16: the folded pipeline against the blocked pipeline with explicit LayerNorm passes and against the reference fixture"""
    from oracle import synth
    g = np.load(os.path.join(GOLDEN, 'vit224_b2.npz'))
    sd = synth.make_vit_state(1, (224, 224))
    x = torch.from_numpy(g['x']).to(dev)
    ref = torch.from_numpy(g['s_feat'])
    m = _vit(sd, (224, 224), dev, True)
    assert m.ln_fold
    out_f = m(x)
    m.ln_fold = False
    out_u = m(x)
    ef, eu = _rel(out_f.cpu(), ref), _rel(out_u.cpu(), ref)
    print('bf16 ViT vs fp32 reference fixture: LayerNorm folded %.3e, explicit %.3e, folded vs explicit %.3e' % (ef, eu, _rel(out_f, out_u)))
    assert ef < 5e-2 and _rel(out_f, out_u) < 2e-2


@pytest.mark.parametrize('outliers', [False, True])
def test_layernorm_fold_stress_large_row_mean_and_outlier_channels(dev, outliers):
    """the folded LayerNorm rounds the RAW stream to bf16 before the mean is subtracted, so its error scales with
    |row mean| / row std -- invisible on random-init streams (mean 0.7, std 2), large on a trained ViT's (token offsets, massive-activation
    channels).  Stress streams: row mean = +-20 std; and the same plus 4 outlier channels at 100 std (which dominate the row's spread, for
    every formulation alike).  The GEMM pair LayerNorm -> Linear through (a) the folded form WITH the producer's per-row shift (what the model
    runs), (b) the folded form rounding the raw stream (shift off), (c) the explicit bf16 LayerNorm pass + bf16 GEMM and (d) the bf16x3 pair,
    against float64.  Gates: (a) within 2x of (c) on both streams; (b) shows the failure mode on the mean-only stream (> 3x of (c)): that is
    why the shift exists; (d) stays parity-grade."""
    from whmr_amd import _lib as L
    g = torch.Generator().manual_seed(3)
    M, C, N2 = 1000, 768, 2304
    std = 1.5
    t1 = torch.randn(M, C, generator=g) * std + 20 * std * (torch.rand(M, 1, generator=g) * 0.5 + 0.75) * torch.sign(torch.randn(M, 1, generator=g))
    if outliers:
        t1[:, [7, 300, 511, 700]] += 100 * std * torch.tensor([1.0, -1.0, 1.0, -1.0])
    att = torch.randn(M, C, generator=g).bfloat16()
    wp = (torch.randn(C, C, generator=g) / math.sqrt(C)).bfloat16()
    bp = torch.randn(C, generator=g)
    t0 = t1 - (att.float() @ wp.float().t() + bp)                     # residual stream BEFORE the producer GEMM: the producer re-creates t1
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1, torch.randn(C, generator=g) * 0.2
    w2 = torch.randn(N2, C, generator=g) / math.sqrt(C)
    b2 = torch.randn(N2, generator=g)
    tb = L.to_blocked(t0.to(dev))
    nb = tb.shape[0]
    xhat = torch.empty(nb, C // 8, 32, 8, device=dev, dtype=torch.bfloat16)
    stats = torch.zeros(nb * 32, C // 256, 2, device=dev)
    # (a) producer with the per-row shift = the row means of the stream one residual step earlier (t0), as the model chains them
    L.gemm_blk(L.to_blocked(att.to(dev)), L.to_blocked(wp.to(dev)), tb, M, bias=bp.to(dev), epi=L.EPI_F32_RES, res=tb, xhat=xhat, stats_out=stats,
               shift=torch.cat([t0.mean(1), torch.zeros(nb * 32 - M)]).to(dev))
    got_t1 = L.from_blocked(tb, M).cpu()
    ref = (F.layer_norm(got_t1.double(), (C,), gamma.double(), beta.double(), 1e-6) @ w2.double().t() + b2.double())
    wf = (w2 * gamma[None, :]).bfloat16()
    s, c = wf.float().sum(1), b2 + w2 @ beta
    out = torch.empty(nb, N2 // 8, 32, 8, device=dev, dtype=torch.bfloat16)
    L.gemm_blk(xhat, L.to_blocked(wf.to(dev)), out, M, bias=c.to(dev), epi=L.EPI_BF16, stats_in=stats, colsum=s.to(dev), ln_eps=1e-6)
    e_fold = _rel(L.from_blocked(out, M).double().cpu(), ref)
    # (b) the same pair WITHOUT the shift
    tb2 = L.to_blocked(t0.to(dev))
    L.gemm_blk(L.to_blocked(att.to(dev)), L.to_blocked(wp.to(dev)), tb2, M, bias=bp.to(dev), epi=L.EPI_F32_RES, res=tb2, xhat=xhat, stats_out=stats)
    L.gemm_blk(xhat, L.to_blocked(wf.to(dev)), out, M, bias=c.to(dev), epi=L.EPI_BF16, stats_in=stats, colsum=s.to(dev), ln_eps=1e-6)
    e_raw = _rel(L.from_blocked(out, M).double().cpu(), ref)
    # (c) explicit bf16 pipeline: LayerNorm pass -> bf16 operand -> bf16 GEMM
    h = torch.empty(nb, C // 8, 32, 8, device=dev, dtype=torch.bfloat16)
    L.layernorm_blk(tb, gamma.to(dev), beta.to(dev), h, M, 1e-6)
    L.gemm_blk(h, L.to_blocked(w2.bfloat16().to(dev)), out, M, bias=b2.to(dev), epi=L.EPI_BF16)
    e_explicit = _rel(L.from_blocked(out, M).double().cpu(), ref)
    # (d) bf16x3: explicit LayerNorm into a hi / lo pair, three MFMAs per product
    hl = torch.empty_like(h)
    L.layernorm_blk_x3(tb, gamma.to(dev), beta.to(dev), h, hl, M, 1e-6)
    w2h, w2l = L.split_bf16(w2)
    ol = torch.empty_like(out)
    L.gemm_blk(h, L.to_blocked(w2h.to(dev)), out, M, bias=b2.to(dev), epi=L.EPI_BF16, a_lo=hl, w_lo=L.to_blocked(w2l.to(dev)), out_lo=ol)
    e_x3 = _rel(L.from_blocked(out, M).double().cpu() + L.from_blocked(ol, M).double().cpu(), ref)
    print('LayerNorm-fold stress (row mean 20 std%s): folded+shift %.2e, folded raw %.2e, explicit bf16 %.2e, bf16x3 %.2e'
          % (', 4 channels at 100 std' if outliers else '', e_fold, e_raw, e_explicit, e_x3))
    assert e_x3 < 3e-5
    assert e_fold < 2 * e_explicit + 1e-3, 'the folded LayerNorm must not be worse than the explicit bf16 pass on a large-mean stream'
    if not outliers:
        assert e_raw > 3 * e_explicit, 'stress stream too tame: rounding the raw stream should show here'


def test_vit_ln_fold_shift_chain_on_offset_stream(dev):
    """the model's shift chain end to end: a ViT-B whose pos_embed carries a large per-token offset (every token's stream sits at ~30 std off
    zero through all blocks) -- the folded pipeline must track the explicit-LayerNorm pipeline as closely as on the plain weights"""
    from oracle import synth
    g = np.load(os.path.join(GOLDEN, 'vit224_b2.npz'))
    sd = {k: v.clone() for k, v in synth.make_vit_state(1, (224, 224)).items()}
    off = torch.randn(1, sd['pos_embed'].shape[1], 1, generator=torch.Generator().manual_seed(1)).sign() * 30.0
    sd['pos_embed'] = sd['pos_embed'] + off
    x = torch.from_numpy(g['x']).to(dev)
    m = _vit(sd, (224, 224), dev, True)
    out_f = m(x)
    m.ln_fold = False
    out_u = m(x)
    from whmr_amd.models.pose_vit import ViT
    m32 = ViT(img_size=(224, 224), patch_size=16, embed_dim=768, depth=12, num_heads=12, ratio=1, mlp_ratio=4, qkv_bias=True, numerics='bf16x3')
    m32.load_state_dict(sd, strict=True)
    ref = m32.to(dev).eval()(x)
    ef, eu = _rel(out_f, ref), _rel(out_u, ref)
    print('offset stream (30 std per token): folded+shift %.3e, explicit bf16 LayerNorm %.3e (vs bf16x3)' % (ef, eu))
    assert ef < 2 * eu + 1e-3
