"""Every library call of a blocked bf16 ViT inference forward, and the blocked kernels alone at their edges, checked element by element
against float64 references (tests/bf16_reference.py) with bounds derived from the kernels' own arithmetic:

    |y - r| <= rho_out |r| + (kappa + n_round 2^-8) m + alpha

(a) A recorder (tests/call_recorder.py) wraps every public function of ``whmr_amd._lib`` over ``m(x)``: a top-level call with no handler, or
    with a flag its reference does not model, fails the test, and the number of calls of each kind is asserted per configuration.  The
    LayerNorm fold is a CHAIN (statistics / shift buffers ping-pong between producers and consumers), so the recorder keeps the most recent
    producer's stored stream and applied shift, and every fold consumer is checked twice: per call (from the operands it was given) and in
    its semantic form (LN(stream) . W^T from the stream itself) -- the form that sees a stale or swapped statistics / shift buffer.
(b) gemm_blk (every tile x epilogue), the fold pair, attention_blk, layernorm_blk and patch_im2col_blk at the smallest shapes at which they
    can go wrong.

Every fold check asserts the amplification (E[x^2] + mean^2) / (var + eps) <= 4 of its own inputs (bf16_reference._row_stats), so the
bound cannot become vacuous.  Each test prints its worst error / allowance ratio per operation."""
import inspect
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_reference as R  # noqa: E402
import call_recorder  # noqa: E402

pytestmark = pytest.mark.gpu

TILES = [0x44, 0x55, 0x43, 0x33, 0x32, 0x22, 0x54, 0x21]
EPI_NAME = {R.EPI_BF16: 'bf16', R.EPI_BF16_GELU: 'GELU, bf16', R.EPI_F32_RES: '+ blocked residual, fp32', R.EPI_F32_POS: '+ pos[m % rows], fp32'}


class Checks:
    """worst error / allowance ratio per operation; a ratio above 1 fails at once"""

    def __init__(self):
        self.worst = {}

    def record(self, key, ratio):
        assert ratio <= 1.0, '%s: error exceeds its derived bound (worst ratio %.3g)' % (key, ratio)
        self.worst[key] = max(self.worst.get(key, 0.0), ratio)

    def show(self, title):
        print('\n[%s] worst error / allowance per op:' % title)
        for k in sorted(self.worst):
            print('  %-58s %.3e' % (k, self.worst[k]))


def check_plain(ck, key, out, a, w, M, bias, epi, res=None, res_rows=0):
    r, m, alpha = R.gemm_blk(a, w, M, bias=bias, epi=epi, res=res, res_rows=res_rows)
    ck.record(key, R.check(R.unblock(out, M), r, m, alpha=alpha))


def check_producer(ck, out, M, xhat, stats_out, shift, shift_stats, shift_out):
    """the emission of a folding producer from its live stream -> the shift it applied"""
    p = R.fold_producer(out, M, shift=shift, shift_stats=shift_stats, shift_out=shift_out)
    if shift_out is not None:
        ck.record('fold producer shift_out (fp32)', R.check(shift_out.reshape(-1)[:M], *p['s'], rho_out=R.RHO_F32))
    assert torch.equal(R.unblock(xhat, M), p['xhat']), 'xhat != bf16(fp32(C - s))'
    T = p['stats'][0].shape[1]
    ck.record('fold producer stats (sum o, sum o^2) (fp32)', R.check(stats_out.reshape(-1, T, 2)[:M], *p['stats']))
    return p['s_live']


def consumer_ratios(out, a, w, M, stats_in, colsum, bias, eps, epi, stream, s_live):
    """(per-call ratio, semantic ratio, worst amplification) of one fold consumer"""
    y = R.unblock(out, M)
    r, m, alpha, kappa, amp = R.fold_consumer(a, w, M, stats_in, colsum, bias, eps, epi)
    a1 = R.assert_amplification(amp, 'fold consumer (statistics it was given)')
    rc = R.check(y, r, m, alpha=alpha, kappa=kappa)
    del r, m
    r, m, alpha, kappa, amp = R.fold_semantic(stream, s_live, M, w, bias, eps, epi)
    a2 = R.assert_amplification(amp, 'fold consumer (stream of its producer)')
    return rc, R.check(y, r, m, alpha=alpha, kappa=kappa), max(a1, a2)


# ------------------------------------------------------------------------------------------------------------ (a) every call of a forward

class Recorder(call_recorder.Recorder):
    def __init__(self, L):
        super().__init__(L)
        self.desc = inspect.signature(L._blk_desc)
        self.prod = None                  # (stream the most recent producer stored, shift it applied)
        self.amp = 0.0

    def on_cast_bf16(self, live, s):
        assert torch.equal(self.result, s['src'].to(torch.bfloat16)), 'cast_bf16 is not the single rounding of its source'

    def on_to_blocked(self, live, s):
        assert torch.equal(self.result, R.block(s['t'])), 'to_blocked differs from the layout'

    def on_patch_im2col_blk(self, live, s):
        self._only(live, {'x', 'out', 'patch', 'pad'}, self.sigs['patch_im2col_blk'].parameters)
        assert torch.equal(live['out'], R.patch_im2col_blk(s['x'], s['patch'], s['pad'])), 'patch_im2col_blk differs from the exact gather'
        self.counts['patch_im2col_blk bit-exact'] += 1

    def on_layernorm_blk(self, live, s):
        rows = live['rows']
        (r, m), (rm, mm) = R.layernorm_blk(s['x'], rows, s['weight'], s['bias'], live['eps'])
        if live['out_std']:
            assert live['mean_out'] is None
            self.record('layernorm_blk out_std (fp32 row-major)', R.check(live['out'], r, m))
            self.counts['layernorm_blk out_std'] += 1
        else:
            self.record('layernorm_blk (bf16 operand)', R.check(R.unblock(live['out'], rows), r, m))
        if live['mean_out'] is not None:
            self.record('layernorm_blk mean_out (fp32)', R.check(live['mean_out'][:rows], rm, mm))
            self.counts['layernorm_blk mean_out'] += 1

    def on_attention_blk(self, live, s):
        self._only(live, {'qkv', 'out', 'B', 'N', 'H', 'scale'}, self.sigs['attention_blk'].parameters)
        B, N, H = live['B'], live['N'], live['H']
        r, m = R.attention_blk(s['qkv'], B, N, H, live['scale'])
        self.record('attention_blk (bf16)', R.check(R.unblock(live['out'], B * N), r, m, n_round=R.N_ROUND_ATT_BLK))

    def on_gemm_blk(self, live, s):
        kl = self.desc.bind(live['a'], live['w'], live['out'], live['M'], **live['kw'])
        ks = self.desc.bind(s['a'], s['w'], s['out'], s['M'], **s['kw'])
        kl.apply_defaults()
        ks.apply_defaults()
        kl, ks = kl.arguments, ks.arguments
        self._only(kl, {'a', 'w', 'out', 'M', 'bias', 'epi', 'res', 'res_rows', 'tile', 'xhat', 'stats_out', 'stats_in', 'colsum', 'ln_eps', 'shift',
                        'shift_stats', 'shift_out'}, self.desc.parameters)
        M, epi, out = kl['M'], kl['epi'], kl['out']
        if kl['stats_in'] is not None:
            assert kl['xhat'] is None and epi in (R.EPI_BF16, R.EPI_BF16_GELU)
            assert self.prod is not None, 'fold consumer without a live producer in front of it'
            rc, rs, amp = consumer_ratios(out, ks['a'], ks['w'], M, ks['stats_in'], ks['colsum'], ks['bias'], kl['ln_eps'], epi, *self.prod)
            self.amp = max(self.amp, amp)
            self.record('gemm_blk fold consumer, per call (%s)' % EPI_NAME[epi], rc)
            self.record('gemm_blk fold consumer, semantic (%s)' % EPI_NAME[epi], rs)
            self.record('fold colsum = sum_k W\' (fp32)', R.check(ks['colsum'], *R.fold_colsum(ks['w']), kappa=R.KAPPA_SUM))
            self.counts['fold consumer (%s)' % EPI_NAME[epi]] += 1
            return
        check_plain(self, 'gemm_blk (%s)' % EPI_NAME[epi], out, ks['a'], ks['w'], M, ks['bias'], epi, ks['res'], kl['res_rows'])
        if kl['xhat'] is not None:
            s_live = check_producer(self, out, M, kl['xhat'], kl['stats_out'], ks['shift'], ks['shift_stats'], kl['shift_out'])
            self.prod = (out.clone(), s_live.clone())
            self.counts['fold producer xhat bit-exact'] += 1
            self.counts['fold producer (%s)' % ' + '.join(k for k in ('shift', 'shift_stats', 'shift_out') if kl[k] is not None)] += 1
        elif epi >= R.EPI_F32_RES:
            self.prod = None              # the stream moved on without an emission: no consumer may follow


CONFIGS = {
    # name: (img size, batch, embed dim, heads, depth, ln_fold)
    'vitb_224_b64_d2_fold': ((224, 224), 64, 768, 12, 2, True),
    'vitb_224_b11_d2_fold': ((224, 224), 11, 768, 12, 2, True),
    'vitl_256x192_b32_d2_fold': ((256, 192), 32, 1024, 16, 2, True),
    'vitb_256x192_b16_d1_nofold': ((256, 192), 16, 768, 12, 1, False),
}


@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_vit_blocked_bf16_forward_calls_vs_float64(dev, cfg, monkeypatch):
    from oracle import synth
    from whmr_amd import _lib as L
    from whmr_amd.models.pose_vit import ViT
    size, B, D, H, depth, fold = CONFIGS[cfg]
    sd = synth.make_vit_state(21, size, embed_dim=D, depth=depth)
    x = synth.make_inputs(B, 22, size)['x'].to(dev)
    m = ViT(img_size=size, embed_dim=D, depth=depth, num_heads=H, qkv_bias=True, numerics='bf16')
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    m.ln_fold = fold
    assert m.blocked and not m.mx_pilot
    N = (size[0] // 16) * (size[1] // 16)
    M = B * N
    assert M >= m.blocked_min_tokens
    rec = Recorder(L)
    rec.install(monkeypatch)
    out = m(x)
    torch.cuda.synchronize(dev)
    monkeypatch.undo()
    assert out.shape == (B, D, size[0] // 16, size[1] // 16) and torch.isfinite(out).all()
    nw = 1 + 4 * depth                                                 # weight operands made on the first forward: cast to bf16, packed
    want = {'patch_im2col_blk': 1, 'patch_im2col_blk bit-exact': 1, 'cast_bf16': nw, 'to_blocked': nw, 'gemm_blk': nw, 'attention_blk': depth,
            'layernorm_blk out_std': 1}
    if fold:
        # explicit first LayerNorm (mean_out) + unfolded qkv; proj of block 0 with `shift` only, every later producer with shift + shift_stats;
        # folded fc1 in every block and folded qkv from block 1 on; the last fc2 without emission
        want.update({'layernorm_blk': 2, 'layernorm_blk mean_out': 1, 'fold producer xhat bit-exact': 2 * depth - 1,
                     'fold producer (shift + shift_out)': 1, 'fold producer (shift + shift_stats + shift_out)': 2 * depth - 2,
                     'fold consumer (GELU, bf16)': depth, 'fold consumer (bf16)': depth - 1})
    else:
        want.update({'layernorm_blk': 2 * depth + 1})
    got = {k: v for k, v in rec.counts.items() if v}
    assert got == {k: v for k, v in want.items() if v}, (got, want)
    print('\n[%s] M = %d, N = %d, worst fold amplification %.3f; worst error / allowance per op:' % (cfg, M, N, rec.amp))
    for line in rec.table():
        print(line)


# ------------------------------------------------------------------------------------------------------- (b) single kernels at their edges

@pytest.mark.parametrize('M,N,K', [(1000, 256, 32), (1001, 512, 64), (777, 256, 96), (392, 768, 768)])
@pytest.mark.parametrize('tile', [0] + TILES)
def test_gemm_blk_epilogues_vs_float64(dev, M, N, K, tile):
    """every tile (0 = the chooser) x the four epilogues; K of 1 / 2 / 3 half tiles (the ring prologue) and 24; M tails inside a 32-row
    block and inside a tile; rows >= M of the last block are not compared"""
    from whmr_amd import _lib as L
    g = torch.Generator().manual_seed(M + N + K + tile)
    a = torch.randn(M, K, generator=g).bfloat16().to(dev)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    res = L.to_blocked(torch.randn(M, N, generator=g).to(dev))
    pos = torch.randn(196, N, generator=g).to(dev)
    ab, wb = L.to_blocked(a), L.to_blocked(w)
    nb = ab.shape[0]
    ck = Checks()
    out = torch.full((nb, N // 8, 32, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    for epi, b in ((L.EPI_BF16, bias), (L.EPI_BF16, None), (L.EPI_BF16_GELU, bias)):
        L.gemm_blk(ab, wb, out, M, bias=b, epi=epi, tile=tile)
        check_plain(ck, 'gemm_blk (%s)' % EPI_NAME[epi], out, ab, wb, M, b, epi)
    t = res.clone()
    L.gemm_blk(ab, wb, t, M, bias=bias, epi=L.EPI_F32_RES, res=t, tile=tile)                     # in place
    check_plain(ck, 'gemm_blk (%s)' % EPI_NAME[L.EPI_F32_RES], t, ab, wb, M, bias, L.EPI_F32_RES, res)
    t2 = torch.full((nb, N // 4, 32, 4), float('nan'), device=dev)
    L.gemm_blk(ab, wb, t2, M, bias=bias, epi=L.EPI_F32_POS, res=pos, res_rows=196, tile=tile)
    check_plain(ck, 'gemm_blk (%s)' % EPI_NAME[L.EPI_F32_POS], t2, ab, wb, M, bias, L.EPI_F32_POS, pos, 196)
    ck.show('gemm_blk M %d N %d K %d tile %#x' % (M, N, K, tile))


def _fold_inputs(dev, N1, form, seed, M=1000, K0=64, N2=512, std=2.0):
    """a residual stream t1 (re-created by the producer as t0 + att . wp^T + bp) and the folded Linear behind it.  With a shift the rows of t1
    sit at +-20 std and the shift (the row means of t0, as the model chains them) centres them; without one only a nearly centred stream
    (mean 0.7, std 2: amplification 1.25) meets the condition."""
    from whmr_amd import _lib as L
    g = torch.Generator().manual_seed(seed)
    att = torch.randn(M, K0, generator=g).bfloat16()
    wp = (torch.randn(N1, K0, generator=g) / math.sqrt(K0)).bfloat16()
    bp = torch.randn(N1, generator=g)
    if form == 'none':
        t1 = torch.randn(M, N1, generator=g) * std + 0.7
    else:
        t1 = torch.randn(M, N1, generator=g) * std + 20 * std * torch.sign(torch.randn(M, 1, generator=g))
    t0 = t1 - (att.float() @ wp.float().t() + bp)
    gamma, beta = torch.randn(N1, generator=g) * 0.3 + 1, torch.randn(N1, generator=g) * 0.2
    w2 = torch.randn(N2, N1, generator=g) / math.sqrt(N1)
    wf = (w2 * gamma).bfloat16()
    nb = (M + 31) // 32
    pad = lambda v: torch.cat([v, torch.zeros(nb * 32 - M)]).to(dev)
    k = dict(M=M, N1=N1, N2=N2, nb=nb, att=L.to_blocked(att.to(dev)), wp=L.to_blocked(wp.to(dev)), bp=bp.to(dev), t0=L.to_blocked(t0.to(dev)),
             wf=L.to_blocked(wf.to(dev)), colsum=wf.float().sum(1).to(dev), c=(torch.randn(N2, generator=g) + w2 @ beta).to(dev),
             shift=None, shift_stats=None, shift_out=None)
    if form != 'none':
        mu0 = t0.mean(1)
        if form == 'shift':
            k['shift'] = pad(mu0)
        else:
            # an older shift + the sums taken relative to it, as a producer in the middle of the chain finds them
            old = mu0 - 0.25 * std
            part = (t0 - old.view(-1, 1)).view(M, N1 // 256, 256).sum(-1)
            k['shift'] = pad(old)
            k['shift_stats'] = torch.cat([torch.stack([part, part * part], -1), torch.zeros(nb * 32 - M, N1 // 256, 2)]).to(dev).contiguous()
            k['shift_out'] = torch.full((nb * 32,), float('nan'), device=dev)
    return k


def _run_producer(L, dev, k, tile):
    t = k['t0'].clone()
    xhat = torch.full((k['nb'], k['N1'] // 8, 32, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    stats = torch.full((k['nb'] * 32, k['N1'] // 256, 2), float('nan'), device=dev)
    L.gemm_blk(k['att'], k['wp'], t, k['M'], bias=k['bp'], epi=L.EPI_F32_RES, res=t, tile=tile, xhat=xhat, stats_out=stats, shift=k['shift'],
               shift_stats=k['shift_stats'], shift_out=k['shift_out'])
    return t, xhat, stats


@pytest.mark.parametrize('form', ['none', 'shift', 'shift+stats'])
@pytest.mark.parametrize('tile', [0, 0x44, 0x32, 0x55, 0x21])
@pytest.mark.parametrize('N1', [256, 768, 1024])
def test_gemm_blk_fold_pair_vs_float64(dev, N1, tile, form):
    """the folded LayerNorm -> Linear pair: 1, 3 and 4 statistics partials per row, three forms of the producer, both consumers (plain and
    GELU), each consumer per call and in its semantic form; M = 1000 ends inside a 32-row block and inside every tile"""
    from whmr_amd import _lib as L
    k = _fold_inputs(dev, N1, form, 100 + N1 + tile)
    M = k['M']
    ck = Checks()
    t, xhat, stats = _run_producer(L, dev, k, tile)
    check_plain(ck, 'gemm_blk (%s)' % EPI_NAME[L.EPI_F32_RES], t, k['att'], k['wp'], M, k['bp'], L.EPI_F32_RES, k['t0'])
    s_live = check_producer(ck, t, M, xhat, stats, k['shift'], k['shift_stats'], k['shift_out'])
    ck.record('fold colsum = sum_k W\' (fp32)', R.check(k['colsum'], *R.fold_colsum(k['wf']), kappa=R.KAPPA_SUM))
    out = torch.full((k['nb'], k['N2'] // 8, 32, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    amp = 0.0
    for epi in (L.EPI_BF16, L.EPI_BF16_GELU):
        L.gemm_blk(xhat, k['wf'], out, M, bias=k['c'], epi=epi, tile=tile, stats_in=stats, colsum=k['colsum'], ln_eps=1e-6)
        rc, rs, a = consumer_ratios(out, xhat, k['wf'], M, stats, k['colsum'], k['c'], 1e-6, epi, t, s_live)
        amp = max(amp, a)
        ck.record('gemm_blk fold consumer, per call (%s)' % EPI_NAME[epi], rc)
        ck.record('gemm_blk fold consumer, semantic (%s)' % EPI_NAME[epi], rs)
    ck.show('fold pair N1 %d tile %#x producer %s, amplification %.3f' % (N1, tile, form, amp))


def test_fold_semantic_check_sees_a_stale_statistics_buffer(dev):
    """a test of the test, through the public API: the consumer is handed the statistics of ANOTHER stream (what a wrong ping-pong index
    leaves).  The call is correct for the inputs it got -- the per-call form passes -- and the model is wrong: the semantic form fails."""
    from whmr_amd import _lib as L
    k = _fold_inputs(dev, 768, 'shift', 7)
    other = _fold_inputs(dev, 768, 'shift', 8, std=3.0)
    M = k['M']
    t, xhat, stats = _run_producer(L, dev, k, 0)
    _, _, stale = _run_producer(L, dev, other, 0)
    s_live = R.fold_producer(t, M, shift=k['shift'])['s_live']
    out = torch.full((k['nb'], k['N2'] // 8, 32, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    L.gemm_blk(xhat, k['wf'], out, M, bias=k['c'], epi=L.EPI_BF16, stats_in=stats, colsum=k['colsum'], ln_eps=1e-6)
    rc, rs, _ = consumer_ratios(out, xhat, k['wf'], M, stats, k['colsum'], k['c'], 1e-6, L.EPI_BF16, t, s_live)
    assert rc <= 1.0 and rs <= 1.0, (rc, rs)
    L.gemm_blk(xhat, k['wf'], out, M, bias=k['c'], epi=L.EPI_BF16, stats_in=stale, colsum=k['colsum'], ln_eps=1e-6)
    rc2, rs2, _ = consumer_ratios(out, xhat, k['wf'], M, stale, k['colsum'], k['c'], 1e-6, L.EPI_BF16, t, s_live)
    print('\nstale statistics buffer: per call %.3e (own statistics %.3e), semantic %.3e (own statistics %.3e)' % (rc2, rc, rs2, rs))
    assert rc2 <= 1.0 < rs2, (rc2, rs2)


@pytest.mark.parametrize('amp', [1.5, 4.0])
@pytest.mark.parametrize('N,B', [(65, 2), (80, 2), (100, 2), (192, 2), (196, 2), (240, 2), (256, 2), (196, 44)])
def test_attention_blk_vs_float64(dev, N, B, amp):
    """per element, on the persistent 16-row-tile kernel (N <= 240; one real row in the last tile at 65, 15 tiles at 240, up to three items
    per workgroup at B = 44) and the kernel behind it (N = 256, and every N through variant bit 4); score amplitude 4 = a peaked softmax;
    V has a non-zero mean, so a dropped or doubled key does not average out"""
    from whmr_amd import _lib as L
    H = 12
    g = torch.Generator().manual_seed(N + B)
    qkv = (torch.randn(B * N, 3 * H * 64, generator=g) * amp).bfloat16()
    qkv[:, 2 * H * 64:] += 0.75
    qb = L.to_blocked(qkv.to(dev))
    r, m = R.attention_blk(qb, B, N, H, 0.125)
    ck = Checks()

    def run(key):
        out = torch.full((qb.shape[0], H * 8, 32, 8), float('nan'), device=dev, dtype=torch.bfloat16)
        L.attention_blk(qb, out, B, N, H, 0.125)
        ck.record(key, R.check(R.unblock(out, B * N), r, m, n_round=R.N_ROUND_ATT_BLK))
        if (B * N) % 32:
            assert torch.isnan(R.unblock(out, qb.shape[0] * 32)[B * N:].float()).all(), 'rows >= B N of the last block were written'
    run('attention_blk (bf16)')
    L.attention_set_variant(1 | 16)
    try:
        run('attention_blk, variant bit 4 (bf16)')
    finally:
        L.attention_set_variant(1)
    ck.show('attention_blk N %d B %d amplitude %g' % (N, B, amp))


@pytest.mark.parametrize('stream', ['mean 0.5 std 3', 'mean 20 std'])
@pytest.mark.parametrize('C', [256, 768, 1024, 1280])
def test_layernorm_blk_vs_float64(dev, C, stream):
    """the bf16 operand form (with and without mean_out), the fp32 row-major form and the row means; 391 rows end inside a block"""
    from whmr_amd import _lib as L
    g = torch.Generator().manual_seed(C)
    rows = 391
    if stream == 'mean 20 std':
        x = torch.randn(rows, C, generator=g) * 1.5 + 30.0 * torch.sign(torch.randn(rows, 1, generator=g))
    else:
        x = torch.randn(rows, C, generator=g) * 3 + 0.5
    w, b = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    xb = L.to_blocked(x.to(dev))
    (r, m), (rm, mm) = R.layernorm_blk(xb, rows, w, b, 1e-6)
    ck = Checks()
    out = torch.full((xb.shape[0], C // 8, 32, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    L.layernorm_blk(xb, w, b, out, rows, 1e-6)
    ck.record('layernorm_blk (bf16 operand)', R.check(R.unblock(out, rows), r, m))
    out2 = torch.full_like(out, float('nan'))
    mean = torch.full((xb.shape[0] * 32,), float('nan'), device=dev)
    L.layernorm_blk(xb, w, b, out2, rows, 1e-6, mean_out=mean)
    assert torch.equal(R.unblock(out2, rows), R.unblock(out, rows))
    ck.record('layernorm_blk mean_out (fp32)', R.check(mean[:rows], rm, mm))
    std = torch.full((rows, C), float('nan'), device=dev)
    L.layernorm_blk(xb, w, b, std, rows, 1e-6, out_std=True)
    ck.record('layernorm_blk out_std (fp32 row-major)', R.check(std, r, m))
    ck.show('layernorm_blk C %d, %s' % (C, stream))


@pytest.mark.parametrize('size', [(224, 224), (256, 192)])
def test_patch_im2col_blk_bit_exact(dev, size):
    """the padded patch grid (pad 2) at batch 3: 588 rows end inside a 32-row block, 576 do not; padding rows are zero"""
    from whmr_amd import _lib as L
    x = torch.randn(3, 3, *size, generator=torch.Generator().manual_seed(size[1])).to(dev)
    M = 3 * (size[0] // 16) * (size[1] // 16)
    out = torch.full(((M + 31) // 32, 96, 32, 8), float('nan'), device=dev, dtype=torch.bfloat16)
    L.patch_im2col_blk(x, out, 16, 2)
    assert torch.equal(out, R.patch_im2col_blk(x, 16, 2))
