"""ViTPose backbone on MI355X -- same module surface as the reference, HIP kernels inside.

Mirrors models/pose_vit.py:8-23 (``VitPose`` with child ``.backbone``, ``get_vitpose_encoder``) and the
``ViT`` of models/ViTPose/mmpose/models/backbones/vit.py:200-341: identical constructor arguments for the
parts W-HMR uses, identical ``state_dict`` keys, ``forward(x) -> [B, C, Hp, Wp]``.

Forward (inference) = 1 im2col + 1 + 12*4 GEMM launches + 25 LayerNorms + 12 attention launches, all from
libwhmr_hip.so.  ``numerics``: 'bf16x3' (DEFAULT -- the reference's ViT is fp32 throughout, vit.py:61-140, and a drop-in must land inside
the 1e-4 contract: split-bf16, every GEMM / attention operand a hi + lo bf16 pair and every product three bf16 MFMAs with fp32
accumulate -- fp32-grade results, ~1e-5 of the reference, at 2.4x the bf16 time instead of 8x; shapes its kernels are not built for run
the 'fp32' path), 'fp32' (exact-f32 MFMA everywhere; also what a 'bf16x3' model trains in) or 'bf16' (the explicit THROUGHPUT opt-in:
bf16 MFMA operands, fp32 accumulate, fp32 residual stream; ~5e-3 of the reference on the feature map).

bf16 inference keeps every activation between the patch gather and the last LayerNorm in the BLOCKED layout of
``csrc/gemm_blk.hip`` ([rows/32][cols/E][32][E]: 512-byte units that are at once an MFMA operand fetch, an MFMA result
and a contiguous run of memory), so the GEMMs need no LDS swizzle / transpose and run the two-group ping-pong schedule;
LayerNorm, the attention core and the patch gather have blocked variants.  ``ViT.blocked = False`` selects the row-major
kernels (same arithmetic; kept for A/B runs, the training graph and the fp32 parity mode use them too).
"""
import math

import os

import torch
import torch.nn as nn

from .. import _lib as L


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class _Holder(nn.Module):
    """Parameter container (keeps reference key names; compute is driven by ViT.forward)."""


def _linear_params(m, name, out_f, in_f, bias=True):
    lin = _Holder()
    lin.weight = nn.Parameter(torch.empty(out_f, in_f))
    nn.init.trunc_normal_(lin.weight, std=.02)
    if bias:
        lin.bias = nn.Parameter(torch.zeros(out_f))
    else:
        lin.register_parameter('bias', None)
    setattr(m, name, lin)


def _ln_params(m, name, dim):
    ln = _Holder()
    ln.weight = nn.Parameter(torch.ones(dim))
    ln.bias = nn.Parameter(torch.zeros(dim))
    setattr(m, name, ln)


class ViT(nn.Module):
    """vit.py:200-341 (plain ViT, pos-embed with an unused cls slot, pre-LN blocks eps 1e-6, last_norm)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=80, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=False, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.,
                 hybrid_backbone=None, norm_layer=None, use_checkpoint=False, frozen_stages=-1, ratio=1,
                 last_norm=True, patch_padding='pad', freeze_attn=False, freeze_ffn=False, numerics='bf16x3'):
        super().__init__()
        assert hybrid_backbone is None and ratio == 1 and last_norm, 'only the configuration W-HMR uses is built'
        img_size, ps = _pair(img_size), _pair(patch_size)
        assert ps[0] == ps[1]
        self.img_size, self.patch_size = img_size, ps[0]
        self.embed_dim = self.num_features = embed_dim
        self.depth, self.num_heads = depth, num_heads
        self.scale = qk_scale or (embed_dim // num_heads) ** -0.5
        assert numerics in ('bf16x3', 'fp32', 'bf16'), numerics
        self.numerics = numerics
        self._eff = 'fp32' if numerics == 'fp32' else 'bf16'      # operand dtype of the row-major path of the current call (set per forward)
        # stochastic depth (vit.py:233): block i drops each of its two residual branches per SAMPLE with probability dpr[i] in training mode
        self.drop_path_rate = float(drop_path_rate)
        self.dpr = [v.item() for v in torch.linspace(0, drop_path_rate, depth)]
        self.drop_masks = None              # test hook: [2*depth, B] 0/1 keep masks used instead of fresh draws (row 2i attention, 2i+1 MLP)
        self.patch_pad = 4 + 2 * (ratio // 2 - 1)                       # vit.py:157 -> 2
        num_patches = (img_size[0] // ps[0]) * (img_size[1] // ps[1])
        self.patch_embed = _Holder()
        self.patch_embed.proj = _Holder()
        self.patch_embed.proj.weight = nn.Parameter(torch.empty(embed_dim, in_chans, ps[0], ps[1]))
        nn.init.kaiming_uniform_(self.patch_embed.proj.weight, a=math.sqrt(5))
        self.patch_embed.proj.bias = nn.Parameter(torch.zeros(embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        nn.init.trunc_normal_(self.pos_embed, std=.02)
        hidden = int(embed_dim * mlp_ratio)
        self.blocks = nn.ModuleList()
        for _ in range(depth):
            blk = _Holder()
            _ln_params(blk, 'norm1', embed_dim)
            blk.attn = _Holder()
            _linear_params(blk.attn, 'qkv', 3 * embed_dim, embed_dim, qkv_bias)
            _linear_params(blk.attn, 'proj', embed_dim, embed_dim)
            _ln_params(blk, 'norm2', embed_dim)
            blk.mlp = _Holder()
            _linear_params(blk.mlp, 'fc1', hidden, embed_dim)
            _linear_params(blk.mlp, 'fc2', embed_dim, hidden)
            self.blocks.append(blk)
        _ln_params(self, 'last_norm', embed_dim)
        self._wcache = {}
        self._ws = {}
        self.blocked = True                 # bf16 inference on the blocked-layout kernels when the shapes allow it
        # pilot, off by default: the four Linears of every block as MXFP8 GEMMs (_forward_tokens_mx) in the bf16 inference path.  NOT a numerics mode:
        # measured slower than bf16 and ~13x its error (profiles/r07_mxfp8_first_measurement.txt); kept to measure the FP8 kernels in the model
        self.mx_pilot = os.environ.get('WHMR_MX_PILOT', '0') != '0'
        self.blocked_min_tokens = 2048      # ... and the batch has at least this many tokens (set 0 to force the blocked path)
        self.x3_min_tokens = 320            # bf16x3: below this many tokens (one 224^2 / 256x192 crop) the exact-f32 path is the faster parity-grade one
        self.ln_fold = True                 # ... with norm1 / norm2 folded into the qkv / fc1 GEMMs (no LayerNorm pass inside the blocks; bf16 and bf16x3)

    # ------------------------------------------------------------------ weight / workspace caches
    def _w(self, p, shape=None, eff=None):
        """Operand copy of a weight in the compute dtype (bf16 copies are re-made when the parameter changes).  ``eff`` ('fp32' | 'bf16'):
        the operand dtype of the CALLER's path; the default is the row-major path of the current eval forward (``self._eff``, set per call) --
        the training forward passes its own (a 'bf16x3' model trains in fp32 whatever the last eval call left in ``_eff``)."""
        if (eff or self._eff) == 'fp32':
            w = p.detach()
            return w.reshape(shape) if shape is not None else w
        key = id(p)
        ent = self._wcache.get(key)
        if ent is None or ent[0] != p._version or ent[1].device != p.device:
            w = L.cast_bf16(p.detach())
            ent = (p._version, w.reshape(shape) if shape is not None else w)
            self._wcache[key] = ent
        return ent[1]

    def _wblk(self, p, shape=None):
        """bf16 copy of a weight [N, K] packed into the blocked operand layout [N/32][K/8][32][8] (re-made when the parameter changes)"""
        key = ('blk', id(p))
        ent = self._wcache.get(key)
        if ent is None or ent[0] != p._version or ent[1].device != p.device:
            w = L.cast_bf16(p.detach())
            ent = (p._version, L.to_blocked(w.reshape(shape) if shape is not None else w))
            self._wcache[key] = ent
        return ent[1]

    def _wfold(self, lin, ln):
        """LayerNorm folded into the Linear that follows it (vit.py:125-126,133-134: lin(LN(x))):
            lin(LN(x))[m, n] = rstd_m * (sum_k x_mk W'_nk - mean_m * s_n) + c_n,   W' = gamma o W,  s_n = sum_k W'_nk,  c_n = b_n + sum_k beta_k W_nk.
        Returns (W' bf16 in the blocked operand layout, s from the ROUNDED W' so that the mean term cancels exactly, c) -- rebuilt when a source changes."""
        srcs = [lin.weight, ln.weight, ln.bias] + ([lin.bias] if lin.bias is not None else [])
        key = ('fold', id(lin.weight))
        ver = tuple((t._version, t.device) for t in srcs)
        ent = self._wcache.get(key)
        if ent is None or ent[0] != ver:
            w = lin.weight.detach().float()
            wp = L.cast_bf16((w * ln.weight.detach().float()[None, :]).contiguous())
            s = wp.float().sum(1).contiguous()
            c = (w.double() @ ln.bias.detach().double()).float()
            if lin.bias is not None:
                c = c + lin.bias.detach().float()
            ent = (ver, (L.to_blocked(wp), s, c.contiguous()))
            self._wcache[key] = ent
        return ent[1]

    def _buf(self, name, shape, dtype, device):
        key = (name, tuple(shape), dtype, device)
        t = self._ws.get(key)
        if t is None:
            t = self._ws[key] = torch.empty(shape, dtype=dtype, device=device)
        return t

    def _pos(self, N, D, device):
        """pos_embed[:, 1:] + pos_embed[:, :1] (vit.py:320) as an [N, D] fp32 table: a constant of the weights, so it is built once per parameter version
        instead of by one framework launch per forward"""
        pe = self.pos_embed
        key = (pe._version, pe.data_ptr(), device, N, D)
        ent = self._ws.get('pos_table')
        if ent is None or ent[0] != key:
            pos = torch.add(pe.detach()[0, 1:], pe.detach()[0, :1]).float().contiguous()
            ent = self._ws['pos_table'] = (key, pos)
        return ent[1]

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward_tokens(self, x):
        """x [B,3,H,W] fp32 (any strides) -> (tokens [B*N, C] fp32 after last_norm, (B, Hp, Wp))."""
        if not x.is_cuda:
            raise RuntimeError('whmr_amd.ViT runs on a HIP device only (no CPU fallback)')
        B, Cin, H, W = x.shape
        P, pad, D = self.patch_size, self.patch_pad, self.embed_dim
        Hp, Wp = (H + 2 * pad - P) // P + 1, (W + 2 * pad - P) // P + 1
        N, M = Hp * Wp, B * Hp * Wp
        assert N + 1 == self.pos_embed.shape[1], 'input size does not match pos_embed (vit.py:231)'
        dev = x.device
        hid_dim = self.blocks[0].mlp.fc1.weight.shape[0] if self.depth else D
        self._eff = 'fp32' if self.numerics == 'fp32' else 'bf16'
        if self.numerics == 'bf16x3':
            if (M >= self.x3_min_tokens and D % 256 == 0 and hid_dim % 256 == 0 and D // self.num_heads == 64 and 64 < N <= 256 and P % 8 == 0
                    and (Cin * P * P) % 32 == 0):
                return self._forward_tokens_x3(x, B, Hp, Wp), (B, Hp, Wp)
            # the split-bf16 kernels are built for the ViTPose shapes (dim % 256 == 0, head dim 64, 64 < tokens <= 256 per image); any other
            # shape keeps the parity-grade contract on the exact-f32 MFMA path below -- and so does ONE crop: a few blocked tiles walk K alone
            # (ViT-B 256x192 at batch 1 under a graph: 2.03 ms split-bf16 vs 1.40 ms exact-f32; from two crops up the split kernels win: 2.1 vs 8.5 ms at 8)
            self._eff = 'fp32'
        dt = torch.float32 if self._eff == 'fp32' else torch.bfloat16
        # below ~2k tokens (batch <= 10 at 192 tokens) the launches are latency-bound and the row-major kernels' smaller tiles + split-K win
        # (ViT-B 256x192 under a HIP graph, tools/smallbatch_probe.py: batch 1 0.85 vs 1.14 ms, batch 8 1.15 vs 1.22, batch 16 1.50 vs 1.32)
        if (self.blocked and M >= self.blocked_min_tokens and self.numerics == 'bf16' and D % 256 == 0 and hid_dim % 256 == 0 and D // self.num_heads == 64
                and 64 < N <= 256 and P % 8 == 0 and (Cin * P * P) % 32 == 0 and D in (256, 768, 1024, 1280)):
            if self.mx_pilot and self.depth:
                return self._forward_tokens_mx(x, B, Hp, Wp), (B, Hp, Wp)
            return self._forward_tokens_blocked(x, B, Hp, Wp), (B, Hp, Wp)
        cols = self._buf('cols', (M, Cin * P * P), dt, dev)
        L.patch_im2col(x.float(), cols, P, pad)
        pos = self._pos(N, D, dev)                                                    # vit.py:320
        t = self._buf('t', (M, D), torch.float32, dev)
        L.gemm(cols, self._w(self.patch_embed.proj.weight, (D, Cin * P * P)), t, bias=self.patch_embed.proj.bias,
               residual=pos, res_row_mod=N)
        h = self._buf('h', (M, D), dt, dev)
        qkv = self._buf('qkv', (M, 3 * D), dt, dev)
        att = self._buf('att', (M, D), dt, dev)
        hid = self._buf('hid', (M, self.blocks[0].mlp.fc1.weight.shape[0]), dt, dev) if self.depth else None
        for blk in self.blocks:
            L.layernorm(t, blk.norm1.weight, blk.norm1.bias, h, 1e-6)
            L.gemm(h, self._w(blk.attn.qkv.weight), qkv, bias=blk.attn.qkv.bias)
            L.attention(qkv, att, B, N, self.num_heads, D // self.num_heads, self.scale)
            L.gemm(att, self._w(blk.attn.proj.weight), t, bias=blk.attn.proj.bias, residual=t)
            L.layernorm(t, blk.norm2.weight, blk.norm2.bias, h, 1e-6)
            L.gemm(h, self._w(blk.mlp.fc1.weight), hid, bias=blk.mlp.fc1.bias, act=L.ACT_GELU)
            L.gemm(hid, self._w(blk.mlp.fc2.weight), t, bias=blk.mlp.fc2.bias, residual=t)
        out = torch.empty((M, D), dtype=torch.float32, device=dev)     # fresh: the caller keeps it (nn.Module value semantics)
        L.layernorm(t, self.last_norm.weight, self.last_norm.bias, out, 1e-6)
        return out, (B, Hp, Wp)

    def _forward_tokens_blocked(self, x, B, Hp, Wp):
        """bf16 inference on the blocked-layout kernels: same arithmetic as the row-major path below the patch gather (bf16 MFMA operands,
        fp32 accumulate, fp32 residual stream, fp32 LayerNorm statistics); only where an element lives in memory differs."""
        Cin, P, pad, D, heads = x.shape[1], self.patch_size, self.patch_pad, self.embed_dim, self.num_heads
        N, M = Hp * Wp, B * Hp * Wp
        nb = (M + 31) // 32
        dev, bf, f32 = x.device, torch.bfloat16, torch.float32
        K0 = Cin * P * P
        cols = self._buf('cols_blk', (nb, K0 // 8, 32, 8), bf, dev)
        L.patch_im2col_blk(x.float(), cols, P, pad)
        pos = self._pos(N, D, dev)                                                    # vit.py:320
        t = self._buf('t_blk', (nb, D // 4, 32, 4), f32, dev)
        fold = self.ln_fold and D <= 1024
        if not fold:
            L.gemm_blk(cols, self._wblk(self.patch_embed.proj.weight, (D, K0)), t, M, bias=self.patch_embed.proj.bias, epi=L.EPI_F32_POS,
                       res=pos, res_rows=N)
        h = self._buf('h_blk', (nb, D // 8, 32, 8), bf, dev)
        qkv = self._buf('qkv_blk', (nb, 3 * D // 8, 32, 8), bf, dev)
        att = self._buf('att_blk', (nb, D // 8, 32, 8), bf, dev)
        hd = self.blocks[0].mlp.fc1.weight.shape[0] if self.depth else D
        hid = self._buf('hid_blk', (nb, hd // 8, 32, 8), bf, dev)
        if fold:
            # LayerNorm folding: the GEMM that produces the residual stream (patch embed, proj, fc2) also writes its bf16 copy h and per-row
            # partial sums; qkv / fc1 multiply that raw copy by gamma-scaled weights and finish the normalisation in their epilogue.  Saves the
            # 2 x depth LayerNorm passes (57.8 MB each at batch 64) for 19 MB of extra stores per producer.
            # The bf16 copy is taken of the CENTRED row: each producer subtracts the row's mean one residual step earlier (previous shift + the
            # mean of the previous shifted statistics; LayerNorm is shift-invariant), so the bf16 rounding is relative to the row's spread and
            # not to its offset (tests/test_blocked_gpu.py::test_layernorm_fold_stress_*).  Statistics / shifts ping-pong between two buffers:
            # a producer's column tiles read the previous pair while they write the next one.
            st = [self._buf('stats%d' % i, (nb * 32, D // 256, 2), f32, dev) for i in (0, 1)]
            sh = [self._buf('shift%d' % i, (nb * 32,), f32, dev) for i in (0, 1)]
            # The FIRST LayerNorm (block 0's norm1) runs as an explicit pass: the patch-embed producer has no earlier statistics to centre its
            # copy with (pos_embed can carry any per-token offset), and that pass hands the chain its first row means.
            nblk = len(self.blocks)
            cur = 0
            L.gemm_blk(cols, self._wblk(self.patch_embed.proj.weight, (D, K0)), t, M, bias=self.patch_embed.proj.bias, epi=L.EPI_F32_POS,
                       res=pos, res_rows=N)
            for bi, blk in enumerate(self.blocks):
                if bi == 0:
                    L.layernorm_blk(t, blk.norm1.weight, blk.norm1.bias, h, M, 1e-6, mean_out=sh[cur])
                    L.gemm_blk(h, self._wblk(blk.attn.qkv.weight), qkv, M, bias=blk.attn.qkv.bias, epi=L.EPI_BF16)
                else:
                    wq, sq, cq = self._wfold(blk.attn.qkv, blk.norm1)
                    L.gemm_blk(h, wq, qkv, M, bias=cq, epi=L.EPI_BF16, stats_in=st[cur], colsum=sq, ln_eps=1e-6)
                L.attention_blk(qkv, att, B, N, heads, self.scale)
                L.gemm_blk(att, self._wblk(blk.attn.proj.weight), t, M, bias=blk.attn.proj.bias, epi=L.EPI_F32_RES, res=t, xhat=h,
                           stats_out=st[cur ^ 1], shift=sh[cur], shift_stats=None if bi == 0 else st[cur], shift_out=sh[cur ^ 1])
                cur ^= 1
                w1, s1, c1 = self._wfold(blk.mlp.fc1, blk.norm2)
                L.gemm_blk(h, w1, hid, M, bias=c1, epi=L.EPI_BF16_GELU, stats_in=st[cur], colsum=s1, ln_eps=1e-6)
                w2 = self._wblk(blk.mlp.fc2.weight)
                if bi + 1 == nblk:
                    L.gemm_blk(hid, w2, t, M, bias=blk.mlp.fc2.bias, epi=L.EPI_F32_RES, res=t)
                else:
                    L.gemm_blk(hid, w2, t, M, bias=blk.mlp.fc2.bias, epi=L.EPI_F32_RES, res=t, xhat=h,
                               stats_out=st[cur ^ 1], shift=sh[cur], shift_stats=st[cur], shift_out=sh[cur ^ 1])
                    cur ^= 1
            out = torch.empty((M, D), dtype=f32, device=dev)
            L.layernorm_blk(t, self.last_norm.weight, self.last_norm.bias, out, M, 1e-6, out_std=True)
            return out
        for blk in self.blocks:
            L.layernorm_blk(t, blk.norm1.weight, blk.norm1.bias, h, M, 1e-6)
            L.gemm_blk(h, self._wblk(blk.attn.qkv.weight), qkv, M, bias=blk.attn.qkv.bias, epi=L.EPI_BF16)
            L.attention_blk(qkv, att, B, N, heads, self.scale)
            L.gemm_blk(att, self._wblk(blk.attn.proj.weight), t, M, bias=blk.attn.proj.bias, epi=L.EPI_F32_RES, res=t)
            L.layernorm_blk(t, blk.norm2.weight, blk.norm2.bias, h, M, 1e-6)
            L.gemm_blk(h, self._wblk(blk.mlp.fc1.weight), hid, M, bias=blk.mlp.fc1.bias, epi=L.EPI_BF16_GELU)
            L.gemm_blk(hid, self._wblk(blk.mlp.fc2.weight), t, M, bias=blk.mlp.fc2.bias, epi=L.EPI_F32_RES, res=t)
        out = torch.empty((M, D), dtype=f32, device=dev)
        L.layernorm_blk(t, self.last_norm.weight, self.last_norm.bias, out, M, 1e-6, out_std=True)
        return out

    def _wmx(self, p):
        """MX operand (e4m3 data, e8m0 scales) of a Linear weight [N, K], quantised on the device (re-made when the parameter changes)"""
        key = ('mx', id(p))
        ent = self._wcache.get(key)
        if ent is None or ent[0] != p._version or ent[1][0].device != p.device:
            ent = (p._version, L.quantize_mx(p.detach().float().contiguous()))
            self._wcache[key] = ent
        return ent[1]

    def _forward_tokens_mx(self, x, B, Hp, Wp):
        """PILOT (``mx_pilot``, bf16 numerics, blocked envelope): the unfolded blocked pipeline with qkv / proj / fc1 / fc2 as MXFP8 GEMMs (e4m3
        operands with one E8M0 scale per 32 elements along K, fp32 accumulate).  The patch embed GEMM, the attention core, the fp32 residual stream, the LayerNorm statistics and last_norm
        keep the arithmetic of the 'bf16' path; LayerNorm writes the MX operand directly, fc1 writes GELU's result as fc2's MX operand, and the bf16
        attention output is quantised by one pass per block."""
        Cin, P, pad, D, heads = x.shape[1], self.patch_size, self.patch_pad, self.embed_dim, self.num_heads
        N, M = Hp * Wp, B * Hp * Wp
        nb = (M + 31) // 32
        dev, bf, f32, u8 = x.device, torch.bfloat16, torch.float32, torch.uint8
        K0 = Cin * P * P
        hd = self.blocks[0].mlp.fc1.weight.shape[0]
        cols = self._buf('cols_blk', (nb, K0 // 8, 32, 8), bf, dev)
        L.patch_im2col_blk(x.float(), cols, P, pad)
        pos = self._pos(N, D, dev)                                                    # vit.py:320
        t = self._buf('t_blk', (nb, D // 4, 32, 4), f32, dev)
        L.gemm_blk(cols, self._wblk(self.patch_embed.proj.weight, (D, K0)), t, M, bias=self.patch_embed.proj.bias, epi=L.EPI_F32_POS,
                   res=pos, res_rows=N)
        mx = lambda name, cols_: (self._buf(name + '_q', (nb, cols_ // 16, 32, 16), u8, dev), self._buf(name + '_s', (nb, cols_ // 128, 32, 4), u8, dev))
        h, atq, hid = mx('mx_h', D), mx('mx_att', D), mx('mx_hid', hd)
        qkv = self._buf('qkv_blk', (nb, 3 * D // 8, 32, 8), bf, dev)
        att = self._buf('att_blk', (nb, D // 8, 32, 8), bf, dev)
        for blk in self.blocks:
            L.layernorm_blk_mx(t, blk.norm1.weight, blk.norm1.bias, h, M, 1e-6)
            L.gemm_blk_mx(h, self._wmx(blk.attn.qkv.weight), qkv, M, bias=blk.attn.qkv.bias, epi=L.MX_EPI_BF16)
            L.attention_blk(qkv, att, B, N, heads, self.scale)
            L.quantize_mx(att, out=atq, rows=M)
            L.gemm_blk_mx(atq, self._wmx(blk.attn.proj.weight), t, M, bias=blk.attn.proj.bias, epi=L.MX_EPI_F32_RES, res=t)
            L.layernorm_blk_mx(t, blk.norm2.weight, blk.norm2.bias, h, M, 1e-6)
            L.gemm_blk_mx(h, self._wmx(blk.mlp.fc1.weight), hid[0], M, bias=blk.mlp.fc1.bias, epi=L.MX_EPI_GELU_MX, out_scale=hid[1])
            L.gemm_blk_mx(hid, self._wmx(blk.mlp.fc2.weight), t, M, bias=blk.mlp.fc2.bias, epi=L.MX_EPI_F32_RES, res=t)
        out = torch.empty((M, D), dtype=f32, device=dev)
        L.layernorm_blk(t, self.last_norm.weight, self.last_norm.bias, out, M, 1e-6, out_std=True)
        return out

    def _wblk_x3(self, p, shape=None):
        """hi / lo bf16 pair of a weight [N, K] (w_hi + w_lo = w to 16 significand bits), both in the blocked operand layout"""
        key = ('blk_x3', id(p))
        ent = self._wcache.get(key)
        if ent is None or ent[0] != p._version or ent[1][0].device != p.device:
            w = p.detach().float()
            hi, lo = L.split_bf16(w.reshape(shape) if shape is not None else w)
            ent = (p._version, (L.to_blocked(hi.contiguous()), L.to_blocked(lo.contiguous())))
            self._wcache[key] = ent
        return ent[1]

    def _wfold_x3(self, lin, ln):
        """``_wfold`` for the bf16x3 numerics: W' = gamma o W as a hi / lo pair (blocked), s = row sums of hi + lo (what the MFMAs multiply), c"""
        srcs = [lin.weight, ln.weight, ln.bias] + ([lin.bias] if lin.bias is not None else [])
        key = ('fold_x3', id(lin.weight))
        ver = tuple((t._version, t.device) for t in srcs)
        ent = self._wcache.get(key)
        if ent is None or ent[0] != ver:
            w = lin.weight.detach().float()
            hi, lo = L.split_bf16((w * ln.weight.detach().float()[None, :]).contiguous())
            s = (hi.double() + lo.double()).sum(1).float().contiguous()
            c = (w.double() @ ln.bias.detach().double()).float()
            if lin.bias is not None:
                c = c + lin.bias.detach().float()
            ent = (ver, (L.to_blocked(hi.contiguous()), L.to_blocked(lo.contiguous()), s, c.contiguous()))
            self._wcache[key] = ent
        return ent[1]

    def _forward_tokens_x3(self, x, B, Hp, Wp):
        """numerics 'bf16x3': the blocked pipeline with every GEMM / attention operand a hi + lo bf16 pair (three MFMAs per product, fp32
        accumulate), erf GELU to fp32 accuracy (8.7e-7 of float64), fp32 residual stream, LayerNorm folded into the GEMM pairs (``ln_fold``; False = explicit fp32 LayerNorm
        passes whose result is split).  Every activation buffer between two kernels exists twice (hi, lo)."""
        Cin, P, pad, D, heads = x.shape[1], self.patch_size, self.patch_pad, self.embed_dim, self.num_heads
        N, M = Hp * Wp, B * Hp * Wp
        nb = (M + 31) // 32
        dev, bf, f32 = x.device, torch.bfloat16, torch.float32
        K0 = Cin * P * P
        pair = lambda name, cols: (self._buf(name + '_hi', (nb, cols // 8, 32, 8), bf, dev), self._buf(name + '_lo', (nb, cols // 8, 32, 8), bf, dev))
        cols = pair('x3cols', K0)
        L.patch_im2col_blk(x.float(), cols[0], P, pad, out_lo=cols[1])
        pos = self._pos(N, D, dev)                                                    # vit.py:320
        t = self._buf('t_blk', (nb, D // 4, 32, 4), f32, dev)
        w = self._wblk_x3(self.patch_embed.proj.weight, (D, K0))
        L.gemm_blk(cols[0], w[0], t, M, bias=self.patch_embed.proj.bias, epi=L.EPI_F32_POS, res=pos, res_rows=N, a_lo=cols[1], w_lo=w[1])
        hd = self.blocks[0].mlp.fc1.weight.shape[0] if self.depth else D
        h, qkv, att, hid = pair('x3h', D), pair('x3qkv', 3 * D), pair('x3att', D), pair('x3hid', hd)
        if self.ln_fold and D <= 1024 and self.depth:
            # LayerNorm folded into the GEMM pair as in the bf16 pipeline, on operand PAIRS: the producers (proj, fc2) also emit the centred row
            # (x - s_m) split into hi / lo + its partial sums, the consumers (qkv, fc1) multiply it by the hi / lo pair of gamma o W and normalise
            # in their epilogue.  The first LayerNorm runs explicitly and seeds the shift.  Saves 2 x depth - 1 LayerNorm passes (13.5 us each).
            st = [self._buf('stats%d' % i, (nb * 32, D // 256, 2), f32, dev) for i in (0, 1)]
            sh = [self._buf('shift%d' % i, (nb * 32,), f32, dev) for i in (0, 1)]
            cur, nblk = 0, len(self.blocks)
            for bi, blk in enumerate(self.blocks):
                if bi == 0:
                    L.layernorm_blk_x3(t, blk.norm1.weight, blk.norm1.bias, h[0], h[1], M, 1e-6, mean_out=sh[cur])
                    w = self._wblk_x3(blk.attn.qkv.weight)
                    L.gemm_blk(h[0], w[0], qkv[0], M, bias=blk.attn.qkv.bias, epi=L.EPI_BF16, a_lo=h[1], w_lo=w[1], out_lo=qkv[1])
                else:
                    wh, wl, sq, cq = self._wfold_x3(blk.attn.qkv, blk.norm1)
                    L.gemm_blk(h[0], wh, qkv[0], M, bias=cq, epi=L.EPI_BF16, a_lo=h[1], w_lo=wl, out_lo=qkv[1], stats_in=st[cur], colsum=sq, ln_eps=1e-6)
                L.attention_blk(qkv[0], att[0], B, N, heads, self.scale, qkv_lo=qkv[1], out_lo=att[1])
                w = self._wblk_x3(blk.attn.proj.weight)
                L.gemm_blk(att[0], w[0], t, M, bias=blk.attn.proj.bias, epi=L.EPI_F32_RES, res=t, a_lo=att[1], w_lo=w[1], xhat=h[0], xhat_lo=h[1],
                           stats_out=st[cur ^ 1], shift=sh[cur], shift_stats=None if bi == 0 else st[cur], shift_out=sh[cur ^ 1])
                cur ^= 1
                wh, wl, s1, c1 = self._wfold_x3(blk.mlp.fc1, blk.norm2)
                L.gemm_blk(h[0], wh, hid[0], M, bias=c1, epi=L.EPI_BF16_GELU, a_lo=h[1], w_lo=wl, out_lo=hid[1], stats_in=st[cur], colsum=s1, ln_eps=1e-6)
                w = self._wblk_x3(blk.mlp.fc2.weight)
                if bi + 1 == nblk:
                    L.gemm_blk(hid[0], w[0], t, M, bias=blk.mlp.fc2.bias, epi=L.EPI_F32_RES, res=t, a_lo=hid[1], w_lo=w[1])
                else:
                    L.gemm_blk(hid[0], w[0], t, M, bias=blk.mlp.fc2.bias, epi=L.EPI_F32_RES, res=t, a_lo=hid[1], w_lo=w[1], xhat=h[0], xhat_lo=h[1],
                               stats_out=st[cur ^ 1], shift=sh[cur], shift_stats=st[cur], shift_out=sh[cur ^ 1])
                    cur ^= 1
            out = torch.empty((M, D), dtype=f32, device=dev)
            L.layernorm_blk(t, self.last_norm.weight, self.last_norm.bias, out, M, 1e-6, out_std=True)
            return out
        for blk in self.blocks:
            L.layernorm_blk_x3(t, blk.norm1.weight, blk.norm1.bias, h[0], h[1], M, 1e-6)
            w = self._wblk_x3(blk.attn.qkv.weight)
            L.gemm_blk(h[0], w[0], qkv[0], M, bias=blk.attn.qkv.bias, epi=L.EPI_BF16, a_lo=h[1], w_lo=w[1], out_lo=qkv[1])
            L.attention_blk(qkv[0], att[0], B, N, heads, self.scale, qkv_lo=qkv[1], out_lo=att[1])
            w = self._wblk_x3(blk.attn.proj.weight)
            L.gemm_blk(att[0], w[0], t, M, bias=blk.attn.proj.bias, epi=L.EPI_F32_RES, res=t, a_lo=att[1], w_lo=w[1])
            L.layernorm_blk_x3(t, blk.norm2.weight, blk.norm2.bias, h[0], h[1], M, 1e-6)
            w = self._wblk_x3(blk.mlp.fc1.weight)
            L.gemm_blk(h[0], w[0], hid[0], M, bias=blk.mlp.fc1.bias, epi=L.EPI_BF16_GELU, a_lo=h[1], w_lo=w[1], out_lo=hid[1])
            w = self._wblk_x3(blk.mlp.fc2.weight)
            L.gemm_blk(hid[0], w[0], t, M, bias=blk.mlp.fc2.bias, epi=L.EPI_F32_RES, res=t, a_lo=hid[1], w_lo=w[1])
        out = torch.empty((M, D), dtype=f32, device=dev)
        L.layernorm_blk(t, self.last_norm.weight, self.last_norm.bias, out, M, 1e-6, out_std=True)
        return out

    def forward_features(self, x):
        if self.training and torch.is_grad_enabled():
            # training: forward keeps its activations, backward = whmr_amd.train.vit_backward (HIP GEMMs / LayerNorm / GELU kernels)
            from ..train import ViTFn
            B, _, H, W = x.shape
            pad, P = self.patch_pad, self.patch_size
            Hp, Wp = (H + 2 * pad - P) // P + 1, (W + 2 * pad - P) // P + 1
            tok = ViTFn.apply(x, self, *self.parameters())
            return tok.view(B, Hp, Wp, self.embed_dim).permute(0, 3, 1, 2)
        tok, (B, Hp, Wp) = self.forward_tokens(x)
        # vit.py:330 returns NCHW; the tokens already are NHWC, so hand back the NCHW *view* (channels-last memory).
        return tok.view(B, Hp, Wp, self.embed_dim).permute(0, 3, 1, 2)

    def forward(self, x):
        return self.forward_features(x)


class VitPose(nn.Module):
    """models/pose_vit.py:8-15."""

    def __init__(self, config):
        super().__init__()
        cfg = dict(config['backbone'] if isinstance(config, dict) else config.backbone)
        cfg.pop('type', None)
        self.backbone = ViT(**cfg)

    def forward(self, x):
        return self.backbone(x)


# models/ViTPose/configs/body/2d_kpt_sview_rgb_img/topdown_heatmap/coco/ViTPose_base_coco_256x192.py:170-182
VITPOSE_BASE_256x192 = dict(img_size=(256, 192), patch_size=16, embed_dim=768, depth=12, num_heads=12, ratio=1,
                            use_checkpoint=False, mlp_ratio=4, qkv_bias=True, drop_path_rate=0.3)
# .../ViTPose_large_coco_256x192.py:46-58
VITPOSE_LARGE_256x192 = dict(img_size=(256, 192), patch_size=16, embed_dim=1024, depth=24, num_heads=16, ratio=1,
                             use_checkpoint=False, mlp_ratio=4, qkv_bias=True, drop_path_rate=0.5)


def get_vitpose_encoder(cfg=None, pretrained='data/pretrained_model/vitpose-b-multi-coco.pth', numerics='bf16x3'):
    """models/pose_vit.py:17-23.  Loads the ViTPose checkpoint when it exists (strict=False like the reference)."""
    import os
    model = VitPose(dict(backbone=dict(VITPOSE_BASE_256x192, numerics=numerics)))
    if pretrained and os.path.exists(pretrained):
        ckpt = torch.load(pretrained, map_location='cpu')
        model.load_state_dict(ckpt['state_dict'], strict=False)
    return model
