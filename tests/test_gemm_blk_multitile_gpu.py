"""The multi-tile launches of the blocked bf16 GEMM (csrc/gemm_blk16_impl.h, MT: a workgroup walks the tiles blockIdx + k grid and fetches the
next tile's first half tiles, bias / colsum and row statistics under the current tile's epilogue) against the one-tile-per-workgroup launches
of the same kernel: the two must agree BIT FOR BIT on the whole blocked output buffer, at every shape at which the walk takes another path.

``whmr_gemm_blk_set_grid(g)``: g > 0 = g workgroups (1, 3 and 8 here: workgroups with one, two and many tiles in one launch, tile counts
that g does not divide, an M-tail tile reached as a second tile), -1 = never multi-tile (the reference side), 0 = the default."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.75                     # exact in bf16; a row block no tile stores keeps it on both sides, a tile one side skips shows
BM = {0x21: 96, 0x22: 128, 0x32: 160, 0x55: 320}


class grid:
    """``with grid(g):`` -- the launches inside run under whmr_gemm_blk_set_grid(g); the default (0) is restored on the way out"""

    def __init__(self, g):
        self.g = g

    def __enter__(self):
        from whmr_amd import _lib as L
        L.lib().whmr_gemm_blk_set_grid(self.g)

    def __exit__(self, *exc):
        from whmr_amd import _lib as L
        L.lib().whmr_gemm_blk_set_grid(0)


def _operands(dev, M, N, K, seed):
    """a, w blocked; bias; and the fold consumer's inputs: the true per-row partial sums of a (K/256 pairs), colsum of w"""
    from whmr_amd import _lib as L
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).bfloat16().to(dev)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().to(dev)
    k = dict(a=L.to_blocked(a), w=L.to_blocked(w), bias=torch.randn(N, generator=g).to(dev), stats=None, colsum=None)
    if K % 256 == 0:
        nb = k['a'].shape[0]
        part = torch.zeros(nb * 32, K // 256, 256, device=dev)
        part[:M] = a.float().view(M, K // 256, 256)
        k['stats'] = torch.stack([part.sum(-1), (part * part).sum(-1)], -1).contiguous()
        k['colsum'] = w.float().sum(1).contiguous()
    return k


def _run(k, M, N, epi, fold, tile, g):
    from whmr_amd import _lib as L
    out = torch.full((k['a'].shape[0], N // 8, 32, 8), SENTINEL, device=k['a'].device, dtype=torch.bfloat16)
    kw = dict(stats_in=k['stats'], colsum=k['colsum'], ln_eps=1e-6) if fold else {}
    with grid(g):
        L.gemm_blk(k['a'], k['w'], out, M, bias=k['bias'], epi=epi, tile=tile, **kw)
    return out


@pytest.mark.parametrize('K', [32, 64, 96, 256, 768])
@pytest.mark.parametrize('tile', [0x21, 0x22, 0x55, 0x32])
def test_multitile_bit_identical_to_one_tile_per_workgroup(dev, tile, K):
    """H = K / 32 = 1, 2, 3 (the look-ahead issues fewer than three stages), 8 and 24; M = 352, 1000, 1001 (the last two end inside a tile and
    inside a 32-row block); N of 1, 2 and 3 column tiles; both bf16 epilogues, each with and without the LayerNorm fold (K % 256 == 0)"""
    from whmr_amd import _lib as L
    n = 0
    for M in (352, 1000, 1001):
        for N in (256, 512, 768):
            k = _operands(dev, M, N, K, M + N + K + tile)
            tiles = -(-M // BM[tile]) * (N // 256)
            for epi in (L.EPI_BF16, L.EPI_BF16_GELU):
                for fold in ((False, True) if K % 256 == 0 else (False,)):
                    want = _run(k, M, N, epi, fold, tile, -1)
                    assert (R.unblock(want, M) != SENTINEL).any(dim=1).all(), 'the reference side left rows unwritten'
                    for g in (1, 3, 8):
                        got = _run(k, M, N, epi, fold, tile, g)
                        assert torch.equal(got, want), ('tile %#x M %d N %d K %d epi %d fold %s: %d tiles on %d workgroups differ from one tile per '
                                                        'workgroup in %d elements' % (tile, M, N, K, epi, fold, tiles, g, (got != want).sum().item()))
                        n += 1
    print('\n[tile %#x K %d] %d multi-tile launches bit-identical' % (tile, K, n))


@pytest.mark.parametrize('epi', [0, 1])
def test_multitile_vs_float64(dev, epi):
    """one case per epilogue (each plain and folded), 16 tiles of 128 rows on 3 workgroups, held to the bounds of tests/bf16_reference.py"""
    M, N, K, tile = 1000, 512, 256, 0x22
    k = _operands(dev, M, N, K, 77 + epi)
    out = _run(k, M, N, epi, False, tile, 3)
    r, m, alpha = R.gemm_blk(k['a'], k['w'], M, bias=k['bias'], epi=epi)
    plain = R.check(R.unblock(out, M), r, m, alpha=alpha)
    out = _run(k, M, N, epi, True, tile, 3)
    r, m, alpha, kappa, amp = R.fold_consumer(k['a'], k['w'], M, k['stats'], k['colsum'], k['bias'], 1e-6, epi)
    R.assert_amplification(amp, 'fold consumer')
    folded = R.check(R.unblock(out, M), r, m, alpha=alpha, kappa=kappa)
    print('\n[epi %d] worst error / allowance: plain %.3e, folded %.3e' % (epi, plain, folded))
    assert plain <= 1.0 and folded <= 1.0, (plain, folded)


def test_fp32_epilogues_are_never_multitile(dev):
    """epi 2 on more tiles than workgroups: the launcher has no multi-tile instantiation to take (launch_blk16: `if constexpr (EPI < 2)`),
    so g = 3 and g = -1 are the same launch and the same bits"""
    from whmr_amd import _lib as L
    M, N, K = 1000, 512, 96
    k = _operands(dev, M, N, K, 5)
    res = L.to_blocked(torch.randn(M, N, generator=torch.Generator().manual_seed(6)).to(dev))
    outs = []
    for g in (-1, 3):
        t = res.clone()
        with grid(g):
            L.gemm_blk(k['a'], k['w'], t, M, bias=k['bias'], epi=L.EPI_F32_RES, res=t, tile=0x22)
        outs.append(t)
    assert torch.equal(outs[0], outs[1])


def _vit_forward(dev, B, depth, g, monkeypatch):
    """output of a ViT-B 224^2 bf16 forward on the blocked kernels (LayerNorm fold on) under set_grid(g) + a copy of what every gemm_blk stored"""
    from oracle import synth
    from whmr_amd import _lib as L
    from whmr_amd.models.pose_vit import ViT
    sd = synth.make_vit_state(21, (224, 224), depth=depth)
    x = synth.make_inputs(B, 22, (224, 224))['x'].to(dev)
    m = ViT(img_size=(224, 224), depth=depth, qkv_bias=True, numerics='bf16')
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    m.blocked_min_tokens = 0
    assert m.blocked and m.ln_fold
    stored, real = [], L.gemm_blk

    def gemm_blk(a, w, out, M, **kw):
        real(a, w, out, M, **kw)
        stored.append(out.clone())
        return out
    monkeypatch.setattr(L, 'gemm_blk', gemm_blk)
    with grid(g):
        y = m(x)
    torch.cuda.synchronize(dev)
    monkeypatch.undo()
    assert len(stored) == 1 + 4 * depth
    return [y] + stored


def test_vit_forward_batch2_depth2_on_3_workgroups(dev, monkeypatch):
    got, want = _vit_forward(dev, 2, 2, 3, monkeypatch), _vit_forward(dev, 2, 2, -1, monkeypatch)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), 'tensor %d of the forward differs (0 = the output, then every gemm_blk result in call order)' % i


def test_vit_forward_batch64_depth1_default_grid(dev, monkeypatch):
    """the one workload-shaped case (one layer): qkv on 441 and fc1 on 480 tiles, the default grid.  (That the multi-tile kernel is what runs at the
    default grid is not visible from here -- on a device whose CU count is not below the tile counts both sides are the same launch; the
    committed kernel trace, profiles/blk_multitile_new_kernel_stats.txt, shows the `<..., true>` instantiations.)"""
    got, want = _vit_forward(dev, 64, 1, 0, monkeypatch), _vit_forward(dev, 64, 1, -1, monkeypatch)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), 'tensor %d of the forward differs (0 = the output, then every gemm_blk result in call order)' % i
