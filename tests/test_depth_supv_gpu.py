"""Depth auxiliary supervision (cfg.MODEL.PyMAF.DEPTH_SUPV_ON) on the MI355X: the inverse-depth rasteriser (csrc/rasterize.hip, whmr_depth_rasterize)
against the analytic known answers and the float64 restatement (tests/depth_reference.py), the loss kernels (csrc/iuv_loss.hip, whmr_depth_loss /
whmr_depth_loss_bwd) and the one autograd node over the 91-channel head output, and the whole training step with the flag on."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import depth_reference as DR
import whmr_loss_reference as WR

pytestmark = pytest.mark.gpu

# Inverse depth where device and reference resolve a pixel to the same face: 4 x the maximum measured on the first device run (docs/kernels.md,
# "Depth target"), capped at 1e-4; values lie in 0.07 .. 0.22
INV_DEPTH_TOL = 8.1e-6          # measured: max 2.017e-6, median 7.1e-9


@contextlib.contextmanager
def flags(aux=True, depth=True):
    from whmr_amd.core.cfgs import cfg
    old = (cfg.MODEL.PyMAF.AUX_SUPV_ON, cfg.MODEL.PyMAF.DEPTH_SUPV_ON)
    cfg.MODEL.PyMAF.AUX_SUPV_ON, cfg.MODEL.PyMAF.DEPTH_SUPV_ON = aux, depth
    try:
        yield cfg
    finally:
        cfg.MODEL.PyMAF.AUX_SUPV_ON, cfg.MODEL.PyMAF.DEPTH_SUPV_ON = old


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def _device_render(dev, verts, faces, want_faces=True):
    from whmr_amd.utils.renderer import Depth_Renderer
    r = Depth_Renderer(focal_length=DR.FOCAL, orig_size=DR.ORIG, output_size=DR.OUT, faces=torch.as_tensor(np.asarray(faces)))
    out, fid = r.verts2depthimg(torch.as_tensor(verts, dtype=torch.float32).to(dev), torch.as_tensor(DR.CAM, dtype=torch.float32).to(dev), want_faces=True)
    assert out.shape == (len(verts), 1) + DR.OUT and out.dtype == torch.float32 and fid.dtype == torch.int32
    return r, out.cpu().numpy().astype(np.float64), fid.cpu().numpy()


def _decided(verts, faces):
    """reference image, face index and the pixels whose coverage is further than 1e-3 px from changing (the fp32 projection moves a vertex by < 2e-5 px)"""
    ref, rfid, margin = DR.rasterize_depth(verts, faces, DR.CAM, DR.FOCAL, DR.ORIG, DR.OUT, want_margin=True)
    return ref, rfid, margin > 1e-3


# ---- rasteriser: known answers ---------------------------------------------------------------------------------------------------------------
def test_rasteriser_tilted_triangle(dev):
    verts, faces, interior, inv = DR.tilted_triangle()
    ref, rfid, decided = _decided(verts, faces)
    r, out, fid = _device_render(dev, verts, faces)
    assert np.array_equal((fid >= 0)[decided], (rfid >= 0)[decided]) and decided.mean() > 0.99
    assert (fid[0][interior] == 0).all()
    err = np.abs(out[0, 0] - inv)[interior].max()
    print('tilted triangle: max |device - analytic| inverse depth %.2e' % err)
    assert err < 1e-6
    assert not out[0, 0][fid[0] < 0].any()
    with pytest.raises(RuntimeError):
        r.verts2depthimg(torch.as_tensor(verts, dtype=torch.float32), torch.as_tensor(DR.CAM, dtype=torch.float32))


def test_rasteriser_blur_band(dev):
    """centres 0.03 px outside an edge are covered (band 0.0614 px) with the clamped-and-renormalised depth; at 0.10 px they are not"""
    verts, faces, (row, cols), inv = DR.edge_triangle(0.03)
    ref, rfid, decided = _decided(verts, faces)
    _, out, fid = _device_render(dev, verts, faces)
    assert decided.all() and np.array_equal(fid >= 0, rfid >= 0)
    assert (fid[0, row, cols] == 0).all() and np.abs(out[0, 0, row, cols] - inv).max() < 1e-6
    assert np.abs(out - ref)[:, 0][rfid >= 0].max() < 1e-6
    verts, faces, (row, cols), _ = DR.edge_triangle(0.10)
    ref, rfid, decided = _decided(verts, faces)
    _, out, fid = _device_render(dev, verts, faces)
    assert decided.all() and np.array_equal(fid >= 0, rfid >= 0)
    assert (fid[0, row] < 0).all() and not out[0, 0, row].any() and (fid[0, row + 1, cols] == 0).all()


def test_rasteriser_depth_order_culling_and_degenerate_faces(dev):
    verts, interior = DR.stacked_triangles()
    for faces in ([[0, 1, 2], [3, 4, 5]], [[3, 4, 5], [0, 1, 2]]):
        ref, rfid, decided = _decided(verts, faces)
        _, out, fid = _device_render(dev, verts, faces)
        assert np.array_equal((fid >= 0)[decided], (rfid >= 0)[decided])
        assert (fid[0][interior] == faces.index([3, 4, 5])).all()                      # the nearer triangle wins whatever the face order
        assert np.abs(out[0, 0][interior] - 1.0 / (DR.TZ - 0.5)).max() < 1e-6
    same = np.concatenate([verts[:, :3], verts[:, :3]], 1)                             # equal depth: the smaller face index wins
    _, _, fid = _device_render(dev, same, [[3, 4, 5], [0, 1, 2]])
    assert (fid[0][interior] == 0).all()
    for scene in (DR.behind_camera_triangle, DR.degenerate_triangle):
        v, f = scene()
        _, out, fid = _device_render(dev, v, f)
        assert (fid < 0).all() and not out.any(), scene.__name__


# ---- rasteriser: the posed mesh of tests/test_raster_gpu.py ------------------------------------------------------------------------------------
def _posed_soup(assets):
    """the synthetic SMPL mesh posed by the oracle with the triangle soup of 13776 faces and the three cameras of
    test_raster_gpu.py::test_iuv_rasterizer_matches_oracle_on_a_posed_mesh"""
    from oracle import smpl as OS
    g = torch.Generator().manual_seed(2)
    B = 3
    rot = torch.eye(3).expand(B, 24, 3, 3).clone()
    verts, _ = OS.smpl_forward(torch.randn(B, 10, generator=g) * 0.5, rot, assets['smpl'])
    vt = assets['smpl']['v_template']
    o1 = torch.argsort((vt[:, 1] * 20).floor() * 1000 + vt[:, 0] * 10)
    o2 = torch.argsort((vt[:, 1] * 20).floor() * 1000 + vt[:, 2] * 10)
    faces = torch.cat([torch.stack([o1[:-2], o1[1:-1], o1[2:]], 1), torch.stack([o2[:-2], o2[2:], o2[1:-1]], 1)])[:13776].to(torch.int32).contiguous()
    cam = torch.tensor([[0.9, 0.0, 0.0], [0.6, 0.2, -0.1], [1.4, -0.05, 0.1]])
    return verts.float(), faces, cam


def test_rasteriser_matches_the_float64_reference_on_a_posed_mesh(dev, assets):
    from whmr_amd.utils.renderer import Depth_Renderer
    verts, faces, cam = _posed_soup(assets)
    r = Depth_Renderer(orig_size=(256, 256), output_size=(128, 128), faces=faces)
    out, fid = r.verts2depthimg(verts.to(dev), cam.to(dev), want_faces=True)
    assert out.shape == (3, 1, 128, 128)
    ref, rfid = DR.rasterize_depth(verts.numpy(), faces.numpy(), cam.numpy(), 1000.0, (256, 256), (128, 128))
    o, f = out.cpu().numpy().astype(np.float64), fid.cpu().numpy()
    covered = (rfid >= 0).mean()
    differ = (f != rfid).mean()
    agree = (f == rfid) & (rfid >= 0)
    err = np.abs(o - ref)[:, 0][agree]
    print('covered %.3f of the pixels; face index differs on %.2e of them; inverse depth where it agrees: max %.3e median %.3e, values %.3f .. %.3f'
          % (covered, differ, err.max(), np.median(err), ref[:, 0][rfid >= 0].min(), ref[:, 0][rfid >= 0].max()))
    assert covered > 0.02
    assert differ < 2e-3                                                               # the project's cap for fp32 against float64 (tests/test_raster_gpu.py)
    assert err.max() < INV_DEPTH_TOL
    assert not o[:, 0][f < 0].any()                                                    # background exactly 0
    out2 = r.verts2depthimg(verts.to(dev), cam.to(dev))
    assert torch.equal(out, out2)                                                      # deterministic


def _iuv_loss_reference(logits, img, w):
    """core/trainer.py:273-297 on utils/iuvmap.py:67-110 targets (the oracle's maps), float64 on the host, as tests/test_raster_gpu.py states it"""
    import torch.nn.functional as F
    from oracle import raster as OR
    U, V, I, A = (torch.from_numpy(a) for a in OR.iuv_img2map(img.double().numpy()))
    y = logits.double().requires_grad_(True)
    u, v, idx, ann = (t.permute(0, 3, 1, 2) for t in torch.split(y, [25, 25, 25, 15], dim=-1))
    B = y.shape[0]
    li = F.cross_entropy(idx.permute(0, 2, 3, 1).reshape(-1, 25), I.argmax(1).view(-1))
    la = F.cross_entropy(ann.permute(0, 2, 3, 1).reshape(-1, 15), A.argmax(1).view(-1))
    fg = I > 0
    lu = F.smooth_l1_loss(u[fg], U[fg], reduction='sum') / B * w
    lv = F.smooth_l1_loss(v[fg], V[fg], reduction='sum') / B * w
    return y, torch.stack([lu, lv, li, la])


# ---- loss kernels --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loss_case():
    """B = 3, H = 13, W = 11 (P = 429: ragged last block of both kernels), IUV and depth targets as strided crop views, 91 channels with the depth
    channel x 1.5 (both sides of the smooth-L1 knee), sample 1 masked; float64 references of the five terms and their gradient, computed once"""
    g = torch.Generator().manual_seed(11)
    B, H, W, w = 3, 13, 11, 0.125
    part = torch.randint(0, 25, (B, H, W + 8), generator=g).float()
    iuv_full = torch.stack([part / 24.0, torch.rand(B, H, W + 8, generator=g), torch.rand(B, H, W + 8, generator=g)], 1)
    depth_full = torch.rand(B, 1, H, W + 8, generator=g) * 0.3
    y = torch.randn(B, H, W, 91, generator=g) * 1.5
    y = y.bfloat16().float()                                                            # representable in both dtypes
    valid = (1.0, 0.0, 1.0)
    up = torch.tensor([2.0, 0.5, 3.0, 1.5, 0.75])
    ref_y, ref4 = _iuv_loss_reference(y[..., :90], iuv_full[:, :, :, 4:-4], w)
    (ref4 * up[:4].double()).sum().backward()
    grad = torch.zeros(B, H, W, 91, dtype=torch.float64)
    grad[..., :90] = ref_y.grad
    pred = y[..., 90].unsqueeze(1).numpy()
    ld, gd = DR.depth_loss(pred, depth_full[:, :, :, 4:-4].numpy(), valid, w)
    grad[..., 90] = torch.from_numpy(gd[:, 0]) * up[4].item()
    assert (np.abs(pred - depth_full[:, :, :, 4:-4].numpy()) > 1).any()
    ref = torch.cat([ref4.detach(), torch.tensor([ld], dtype=torch.float64)])
    return dict(B=B, H=H, W=W, w=w, iuv=iuv_full, depth=depth_full, y=y, valid=valid, up=up, ref=ref, grad=grad)


def _on_device(c, dtype, dev):
    B, H, W = c['B'], c['H'], c['W']
    if dtype == 'bf16':
        buf = torch.zeros(B * H * W, 128, dtype=torch.bfloat16, device=dev)
        buf[:, :91] = c['y'].view(-1, 91).to(dev)
        y = buf.view(B, H, W, 128)[..., :91]
    else:
        y = c['y'].to(dev)
    iuv, depth = c['iuv'].to(dev)[:, :, :, 4:-4], c['depth'].to(dev)[:, :, :, 4:-4]
    assert not iuv.is_contiguous() and not depth.is_contiguous() and y.stride(2) == (128 if dtype == 'bf16' else 91)
    return y.detach().requires_grad_(True), iuv, depth


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_aux_loss_node_matches_the_float64_formulas(dev, dtype):
    from whmr_amd import _lib as L
    from whmr_amd.train.aux_supervision import AuxLossFn
    c = _loss_case()
    B, H, W, w = c['B'], c['H'], c['W'], c['w']
    y, iuv, depth = _on_device(c, dtype, dev)
    has = torch.tensor(c['valid'], device=dev)
    out = AuxLossFn.apply(y, iuv, depth, has, w)
    print('five terms', out.tolist(), 'reference', c['ref'].tolist())
    assert out.shape == (5,) and torch.allclose(out.cpu().double(), c['ref'], rtol=2e-6, atol=0)
    raw = []
    y.register_hook(raw.append)                                                         # the gradient as the node returns it (a view of its buffer)
    (out * c['up'].to(dev)).sum().backward()
    got, want = y.grad.float().cpu().double(), c['grad']
    scale = want.abs().max()
    tol = 2e-6 if dtype == 'fp32' else 2.0 ** -8                                        # the IUV test's bounds (bf16: one rounding of each entry)
    worst = ((got - want).abs() - tol * want.abs()).max() / scale
    print('gradient: worst excess over the relative bound, in units of the largest entry: %.2e' % worst)
    assert ((got - want).abs() <= tol * want.abs() + 1e-7 * scale).all()
    assert not got[1, :, :, 90].any() and got[0, :, :, 90].abs().max() > 0              # the masked sample's depth gradient is exactly 0
    # the buffer behind the gradient: columns 0..89 are whmr_iuv_losses_bwd's bits, column 90 the depth gradient, the padding zero
    ld = y.stride(2)
    base = raw[0]._base
    assert base is not None and base.numel() == B * H * W * ld and getattr(base, 'whmr_zero_padded', None) == ld
    base = base.view(B * H * W, ld)
    alone = L.iuv_losses_bwd(y.detach()[..., :90], iuv, w, c['up'][:4].to(dev), ld)
    assert torch.equal(base[:, :90], alone[:, :90]) and not alone[:, 90:].any()
    assert torch.equal(base[:, 90], y.grad.reshape(-1, 91)[:, 90]) and not base[:, 91:].any()
    # the loss entry alone, and its column-only backward: nothing but column 90 is touched
    one = L.depth_loss(y.detach(), 90, depth, has, w)
    assert torch.equal(one, out.detach()[4:])
    canvas = torch.full((B * H * W, ld), 7.0, dtype=y.dtype, device=dev)
    L.depth_loss_bwd(y.detach(), 90, depth, has, w, c['up'][4:].to(dev), canvas)
    assert torch.equal(canvas[:, 90], base[:, 90]) and (canvas[:, :90] == 7.0).all() and (canvas[:, 91:] == 7.0).all()
    # has_smpl = None: every sample counts
    ref_all, _ = DR.depth_loss(c['y'][..., 90].unsqueeze(1).numpy(), c['depth'][:, :, :, 4:-4].numpy(), None, w)
    assert abs(L.depth_loss(y.detach(), 90, depth, None, w).item() - ref_all) <= 2e-6 * ref_all
    # deterministic
    y2 = y.detach().clone().requires_grad_(True) if dtype == 'fp32' else y.detach().requires_grad_(True)
    out2 = AuxLossFn.apply(y2, iuv, depth, has, w)
    (out2 * c['up'].to(dev)).sum().backward()
    assert torch.equal(out2.detach(), out.detach()) and torch.equal(y2.grad, y.grad)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_all_invalid_mask_and_zero_weight_give_exact_zeros(dev, dtype):
    from whmr_amd.train.aux_supervision import AuxLossFn
    c = _loss_case()
    y, iuv, depth = _on_device(c, dtype, dev)
    for has, w in ((torch.zeros(3, device=dev), c['w']), (torch.ones(3, device=dev), 0.0)):
        y.grad = None
        out = AuxLossFn.apply(y, iuv, depth, has, w)
        assert out[4].item() == 0.0 and torch.isfinite(out).all()
        (out * c['up'].to(dev)).sum().backward()
        assert not y.grad[..., 90].any() and y.grad[..., 50:90].abs().max() > 0


def test_depth_losses_map_form_matches_the_kernel(dev):
    """the reference-signature form (torch ops on the lazy NCHW view) against whmr_depth_loss on the same channels-last tensor"""
    from whmr_amd import _lib as L
    from whmr_amd.core.cfgs import cfg
    from whmr_amd.train.aux_supervision import DepthHeadOutput, depth_losses
    c = _loss_case()
    y, _, depth = _on_device(c, 'fp32', dev)
    w = float(cfg.LOSS.POINT_REGRESSION_WEIGHTS)
    has = torch.tensor(c['valid'], device=dev)
    d = DepthHeadOutput(y, 90)
    a = depth_losses(d, depth, has)
    b = L.depth_loss(y.detach(), 90, depth, has, w)
    assert d.shape == (3, 1, 13, 11) and abs(a.item() - b.item()) <= 2e-6 * abs(b.item())
    a.backward()
    assert not y.grad[..., :90].any() and y.grad[..., 90].abs().max() > 0


# ---- through the head convolution ---------------------------------------------------------------------------------------------------------------
def test_fused_node_through_the_91_channel_head_convolution(dev):
    """ConvNHWCFn over 91 output channels (bf16: padded to 128) -> AuxLossFn, its padded gradient taken by the convolution's backward as is, against the
    map form (lazy NCHW views -> body_uv_losses + depth_losses through torch autograd); channels 0..89 against the 90-channel convolution"""
    from whmr_amd.core.cfgs import cfg
    from whmr_amd.train import heads_autograd as HA
    from whmr_amd.train.aux_supervision import AuxLossFn, DepthHeadOutput, IUVHeadOutput, body_uv_losses, depth_losses
    from whmr_amd.utils.iuvmap import iuv_img2map
    g = torch.Generator().manual_seed(7)
    B, H, W, Cin = 2, 16, 12, 256
    x = (torch.randn(B, H, W, Cin, generator=g) * 0.5).to(dev).bfloat16()
    part = torch.randint(0, 25, (B, H, W), generator=g).float()
    img = torch.stack([part / 24.0, torch.rand(B, H, W, generator=g), torch.rand(B, H, W, generator=g)], 1).to(dev)
    depth = (torch.rand(B, 1, H, W, generator=g) * 0.3).to(dev)
    has = torch.tensor([1.0, 0.0], device=dev)
    w = float(cfg.LOSS.POINT_REGRESSION_WEIGHTS)
    w91 = torch.randn(91, Cin, 3, 3, generator=torch.Generator().manual_seed(9)) * 0.02
    w91[90] *= 8.0                                                                      # depth predictions on both sides of the knee
    res, hits = [], []
    orig = HA._padded_base
    HA._padded_base = lambda *a_: hits.append(orig(*a_)) or hits[-1]
    try:
        for fused in (True, False):
            wt = w91.to(dev).requires_grad_(True)
            bs = torch.zeros(91, device=dev).requires_grad_(True)
            xin = x.clone().requires_grad_(True)
            y = HA.ConvNHWCFn.apply(xin, wt, 1, torch.bfloat16, 1, bs)
            assert y.shape == (B, H, W, 91) and y.stride(2) == 128
            dp, dd = IUVHeadOutput(y[..., :90], full=y), DepthHeadOutput(y, 90)
            if fused:
                terms = AuxLossFn.apply(y, img, depth, has, w)
                assert dict.__len__(dp) == 0 and dd._map is None                        # nothing materialised
            else:
                lu, lv, li, la = body_uv_losses(dp['predict_u'], dp['predict_v'], dp['predict_uv_index'], dp['predict_ann_index'], iuv_img2map(img))
                terms = torch.stack([lu, lv, li, la, depth_losses(dd, depth, has)])
            loss = terms.sum()
            loss.backward()
            assert (hits[-1] is not None) == fused                                       # fused: the convolution took the node's buffer as is
            res.append((loss.item(), terms.detach().clone(), wt.grad.clone(), bs.grad.clone(), xin.grad.float().clone(), y.detach().clone(), dp.nhwc.stride()))
    finally:
        HA._padded_base = orig
    (lf, tf, wf, bf, xf, yf, st), (lm, tm, wm, bm, xm, _, _) = res
    print('loss fused %.8f map %.8f; terms' % (lf, lm), tf.tolist(), tm.tolist())
    assert abs(lf - lm) < 1e-5 * abs(lm) and tf[4].item() > 0
    for a, b in ((wf, wm), (bf, bm), (xf, xm)):                                          # the existing test's bounds
        assert (a - b).abs().max() <= 2e-2 * b.abs().max() and (a - b).norm() <= 5e-3 * b.norm()
    assert wf[90].abs().max() > 0 and bf[90].abs() > 0                                   # the depth head's own parameters get their gradient
    # channels 0..89 are the 90-channel convolution's bits
    y90 = HA.ConvNHWCFn.apply(x, w91[:90].to(dev), 1, torch.bfloat16, 1, torch.zeros(90, device=dev))
    assert y90.stride() == st and torch.equal(y90, yf[..., :90])      # the same view and strides, the same bits


def test_head_forward_fp32_with_an_odd_leading_dimension(dev):
    """fp32 numerics: npad == Cout == 91 (whmr_gemm_f32, whmr_iuv_losses, whmr_iuv_losses_bwd with ld = 91): channels 0..89 are the 90-channel
    convolution's bits, and the node's gradient reaches the convolution without a padded buffer"""
    from whmr_amd.train import heads_autograd as HA
    from whmr_amd.train.aux_supervision import AuxLossFn, IUVLossFn
    g = torch.Generator().manual_seed(8)
    B, H, W, Cin = 2, 16, 12, 256
    x = (torch.randn(B, H, W, Cin, generator=g) * 0.5).to(dev)
    part = torch.randint(0, 25, (B, H, W), generator=g).float()
    img = torch.stack([part / 24.0, torch.rand(B, H, W, generator=g), torch.rand(B, H, W, generator=g)], 1).to(dev)
    depth = (torch.rand(B, 1, H, W, generator=g) * 0.3).to(dev)
    w91 = (torch.randn(91, Cin, 3, 3, generator=g) * 0.02).to(dev)
    b91 = (torch.randn(91, generator=g) * 0.1).to(dev)
    wt, xin = w91.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y = HA.ConvNHWCFn.apply(xin, wt, 1, torch.float32, 1, b91)
    assert y.stride(2) == 91
    y90 = HA.ConvNHWCFn.apply(x, w91[:90], 1, torch.float32, 1, b91[:90])
    assert torch.equal(y[..., :90].detach(), y90)
    terms = AuxLossFn.apply(y, img, depth, None, 0.125)
    assert torch.equal(terms[:4].detach(), IUVLossFn.apply(y90, img, 0.125))            # the same four values from either layout
    terms.sum().backward()
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w91, b91, padding=1).permute(0, 2, 3, 1)
    assert _rel(y.detach(), ref) < 1e-4
    assert torch.isfinite(wt.grad).all() and wt.grad[90].abs().max() > 0 and xin.grad.abs().max() > 0


def test_depth_head_alone_and_beside_the_iuv_head(dev):
    """dp_head_train concatenates whichever heads exist: the depth head alone (DEPTH_SUPV_ON without AUX_SUPV_ON) through the same ConvNHWCFn, and
    behind the IUV head's 90 channels; the lazy map against torch's convolution, gradients to the head's own parameters"""
    import types
    from whmr_amd.models.whmr import Depth_predict_layer, IUV_predict_layer
    from whmr_amd.train.whmr_train import dp_head_train
    torch.manual_seed(4)
    stub = types.SimpleNamespace(dp_head=IUV_predict_layer(256).to(dev), dpth_head=Depth_predict_layer(256).to(dev), _dt=torch.float32)
    f = (torch.randn(2, 16, 12, 256, generator=torch.Generator().manual_seed(6)) * 0.5).to(dev)
    conv = stub.dpth_head.predict_depth
    want = torch.nn.functional.conv2d(f.permute(0, 3, 1, 2), conv.weight, conv.bias, padding=1).detach()
    dp, dd = dp_head_train(stub, f.clone().requires_grad_(True), False, iuv=False, depth=True)
    assert dp is None and dd.col == 0 and dd.nhwc.shape == (2, 16, 12, 1) and dd.shape == (2, 1, 16, 12) and dd._map is None
    assert _rel(dd.map.detach(), want) < 1e-4
    dd.sum().backward()
    assert conv.weight.grad.abs().max() > 0 and conv.bias.grad.abs().max() > 0
    dp, dd = dp_head_train(stub, f, False, iuv=True, depth=True)
    assert dd.col == 90 and dd.nhwc.shape == (2, 16, 12, 91) and dp.full is dd.nhwc and dp.nhwc.shape == (2, 16, 12, 90)
    assert _rel(dd.map.detach(), want) < 1e-4 and dp['predict_v'].shape == (2, 25, 16, 12)
    only = dp_head_train(stub, f, False)                                                # today's call: the IUV head alone
    assert torch.equal(only.nhwc, dp.nhwc) and only.full is None


# ---- the whole training step ----------------------------------------------------------------------------------------------------------------------
def _train_model(assets, state_dict, dev, depth):
    from whmr_amd.models import whmr_net
    with flags(True, depth):
        m = whmr_net(None, assets=assets, numerics='fp32')
    res = m.load_state_dict(state_dict, strict=False)
    assert not res.unexpected_keys
    assert [k for k in res.missing_keys if '.smpl.' not in k] == (['dpth_head.predict_depth.weight', 'dpth_head.predict_depth.bias'] if depth else [])
    if depth:
        g = torch.Generator().manual_seed(21)
        with torch.no_grad():
            m.dpth_head.predict_depth.weight.copy_(torch.randn(1, 256, 3, 3, generator=g) * 0.02)
            m.dpth_head.predict_depth.bias.fill_(0.1)
    m = m.to(dev).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m.feature_extractor.backbone.drop_path_rate = 0.0
    return m


def _step_inputs(assets, dev):
    from oracle import synth
    from whmr_amd.utils.renderer import Depth_Renderer, IUV_Renderer
    inp = synth.make_inputs(2, 0)
    x = {k: inp[k].to(dev).clone() for k in ('x', 'center', 'scale', 'bbox_height', 'orig_shape', 'bbox_info')}
    _, tgt = WR.make_case(2, (6890, 1723, 431), 7, [1, 0], [1, 1], dtype=torch.float32)
    tgt = {k: v.to(dev) for k, v in tgt.items()}
    batch = {'pose': tgt['gt_pose'], 'betas': tgt['gt_betas'], 'pose_3d': tgt['pose_3d'], 'has_smpl': tgt['has_smpl'], 'has_pose_3d': tgt['has_pose_3d'],
             'opt_vertices': tgt['gt_verts'], 'opt_sub_vertices': tgt['gt_sub_verts'], 'opt_temp_vertices': tgt['gt_temp_verts']}
    _, faces, _ = _posed_soup(assets)
    iuv_maker = IUV_Renderer(orig_size=(256, 256), output_size=(128, 128), dp=synth.make_densepose_tables(0, assets))
    depth_maker = Depth_Renderer(orig_size=(256, 256), output_size=(128, 128), faces=faces)
    gt_cam = torch.tensor([[0.9, 0.0, 0.0], [0.7, 0.1, -0.05]], device=dev)
    return x, batch, iuv_maker, depth_maker, gt_cam


def _make_step(m, x, batch, iuv_maker, depth_maker, gt_cam, params):
    """forward, targets rendered THIS step from the stage-3 mesh (detached; the benchmark's stand-in for the fitted mesh), losses, backward"""
    from whmr_amd.train import compute_losses, total_loss
    from whmr_amd.train.aux_supervision import render_depth_target, render_iuv_targets
    keep = {}

    def step():
        for p_ in params:
            p_.grad = None
        out, _ = m(x['x'], None, x['center'], x['scale'], x['bbox_height'], x['orig_shape'], x['bbox_info'], is_train=True)
        mesh = out['smpl_out'][-1]['verts'].detach()
        t = dict(batch)
        t['iuv_image_gt'], _ = render_iuv_targets(iuv_maker, mesh, gt_cam, maps=False)
        if depth_maker is not None:
            t['depth_image_gt'] = render_depth_target(depth_maker, mesh, gt_cam)
        d = compute_losses(out, t)
        total = total_loss(d)
        total.backward()
        keep.update(out=out, losses=d, targets=t)
        return total
    return step, keep


def test_whole_step_with_the_flag_on(dev, assets, state_dict):
    x, batch, iuv_maker, depth_maker, gt_cam = _step_inputs(assets, dev)
    # flag off: today's step
    with flags(True, False):
        m0 = _train_model(assets, state_dict, dev, False)
        step0, keep0 = _make_step(m0, x, batch, iuv_maker, None, gt_cam, list(m0.parameters()))
        step0()
        assert keep0['out']['dpth_out'] == [] and not hasattr(m0, 'dpth_head') and not any(k.startswith('loss_Depth') for k in keep0['losses'])
        iuv_off = torch.stack([keep0['losses'][k + '-1'] for k in ('loss_U', 'loss_V', 'loss_IndexUV', 'loss_segAnn')]).detach().clone()
    with flags(True, True):
        m = _train_model(assets, state_dict, dev, True)
        params = list(m.parameters())
        step, keep = _make_step(m, x, batch, iuv_maker, depth_maker, gt_cam, params)
        total = step()
        out, d, t = keep['out'], keep['losses'], keep['targets']
        assert len(out['dpth_out']) == 1 and out['dpth_out'][0].shape == (2, 1, 128, 96) and out['dpth_out'][0]._map is None
        assert out['dp_out'][0].nhwc.shape == (2, 128, 96, 90) and out['dp_out'][0].full is out['dpth_out'][0].nhwc
        assert t['depth_image_gt'].shape == (2, 1, 128, 96) and (t['depth_image_gt'] > 0).float().mean() > 0.02
        assert list(d)[:5] == ['loss_U-1', 'loss_V-1', 'loss_IndexUV-1', 'loss_segAnn-1', 'loss_Depth-1']
        assert d['loss_Depth-1'].item() > 0 and len(d.vectors) == 2 and d.vectors[0].shape == (5,)          # ONE node for both heads
        ref_total = torch.stack(list(d.values())).double().sum().item()
        assert abs(total.item() - ref_total) <= 1e-5 * max(1.0, abs(ref_total))
        iuv_on = torch.stack([d[k + '-1'] for k in ('loss_U', 'loss_V', 'loss_IndexUV', 'loss_segAnn')]).detach()
        assert torch.equal(iuv_on, iuv_off)                                            # the depth channel changes no bit of the other 90
        hw, hb = m.dpth_head.predict_depth.weight.grad, m.dpth_head.predict_depth.bias.grad
        assert torch.isfinite(hw).all() and torch.isfinite(hb).all() and hw.abs().max() > 0 and hb.abs().max() > 0
        # the term against the reference-signature form on the lazily created map, on the same forward
        from whmr_amd.train.aux_supervision import depth_losses
        slow = depth_losses(out['dpth_out'][0], t['depth_image_gt'], batch['has_smpl'])
        assert abs(slow.item() - d['loss_Depth-1'].item()) <= 1e-5 * abs(slow.item())
        # inference runs no depth head (the reference computes the map and discards it)
        m.eval()
        eye = torch.eye(3, device=dev).expand(2, 3, 3).contiguous()
        ev, _ = m(x['x'], None, x['center'], x['scale'], x['bbox_height'], x['orig_shape'], x['bbox_info'], cam_rotmat=eye, view='train')
        assert ev['dpth_out'] == [] and ev['dp_out'] == []
        m.train()


def test_whole_step_replays_from_a_captured_graph(dev, assets, state_dict):
    """capture_train_step with the flag on (rasterisers, 91-channel head, AuxLossFn and the objective inside the graph): the replay reproduces the eager
    step's loss and every parameter gradient, as tests/test_train_gpu.py::test_train_step_hip_graph_replay_matches_eager checks for the flag-off step"""
    from oracle import synth
    from whmr_amd.train import capture_train_step
    x, batch, iuv_maker, depth_maker, gt_cam = _step_inputs(assets, dev)
    with flags(True, True):
        m = _train_model(assets, state_dict, dev, True)
        for name, p_ in m.named_parameters():
            if name.startswith(('cam_model', 'global_orient')):
                p_.requires_grad_(False)
        params = [p_ for p_ in m.parameters() if p_.requires_grad]
        step, _ = _make_step(m, x, batch, iuv_maker, depth_maker, gt_cam, params)
        replay, loss = capture_train_step(m, step)
        bn_state = {k: v.clone() for k, v in m.state_dict().items() if 'running' in k}
        for seed in (0, 5):
            new = synth.make_inputs(2, seed)
            for k in x:
                x[k].copy_(new[k].to(dev))
            m.load_state_dict(bn_state, strict=False)
            le = step().item()
            ge = {id(p_): p_.grad.clone() for p_ in params if p_.grad is not None}       # (the default objective leaves a few heads without a loss)
            assert len(ge) > 100 and id(m.dpth_head.predict_depth.weight) in ge and id(m.dp_head.predict_u.weight) in ge
            m.load_state_dict(bn_state, strict=False)
            replay()
            torch.cuda.synchronize()
            assert abs(loss.item() - le) < 1e-5 * max(1.0, abs(le)), (seed, loss.item(), le)
            assert {id(p_) for p_ in params if p_.grad is not None} == set(ge)
            worst = max(_rel(p_.grad, ge[id(p_)]) for p_ in params if id(p_) in ge and ge[id(p_)].abs().max() > 1e-8)
            assert worst < 1e-4, (seed, worst)
        assert m.dpth_head.predict_depth.weight.grad.abs().max() > 0


def test_build_targets_renders_the_depth_image(dev, assets, state_dict):
    """build_targets(depth_maker=): the inverse-depth image of opt_vertices under gt_camera with the vitpose crop, beside the IUV image"""
    from oracle import geometry as OG
    from oracle import smpl as OS
    from oracle import synth
    from whmr_amd.train import build_targets
    from whmr_amd.train.aux_supervision import gt_camera_from_translation
    from whmr_amd.utils.renderer import Depth_Renderer, IUV_Renderer
    with flags(True, True):
        m = _train_model(assets, state_dict, dev, True)
        g = torch.Generator().manual_seed(2)
        pose, betas = torch.randn(2, 72, generator=g) * 0.4, torch.randn(2, 10, generator=g) * 0.5
        _, j_ref = OS.smpl_forward(betas, OG.batch_rodrigues(pose.reshape(-1, 3)).view(2, 24, 3, 3), assets['smpl'])
        cam = j_ref + torch.tensor([[0.1, -0.2, 5.0], [-0.3, 0.2, 8.0]])[:, None]
        px = 1000.0 * cam[..., :2] / cam[..., 2:] + 128.0
        batch = {'pose': pose, 'betas': betas, 'keypoints': torch.cat([px / 112.0 - 1.0, torch.ones(2, 49, 1)], -1), 'has_smpl': torch.ones(2),
                 'has_pose_3d': torch.tensor([1, 0]), 'pose_3d': torch.zeros(2, 24, 4)}
        _, faces, _ = _posed_soup(assets)
        depth_maker = Depth_Renderer(orig_size=(256, 256), output_size=(128, 128), faces=faces)
        iuv_maker = IUV_Renderer(orig_size=(256, 256), output_size=(128, 128), dp=synth.make_densepose_tables(0, assets))
        t = build_targets(m, {k: v.to(dev) for k, v in batch.items()}, iuv_maker=iuv_maker, depth_maker=depth_maker)
        t_iuv_only = build_targets(m, {k: v.to(dev) for k, v in batch.items()}, iuv_maker=iuv_maker)
    assert t['depth_image_gt'].shape == (2, 1, 128, 96) and t['iuv_image_gt'].shape == (2, 3, 128, 96) and 'depth_image_gt' not in t_iuv_only
    assert torch.equal(t['iuv_image_gt'], t_iuv_only['iuv_image_gt'])
    want = depth_maker.verts2depthimg(t['opt_vertices'], gt_camera_from_translation(t['opt_cam_t'], focal_length=1000.0))[:, :, :, 16:-16]
    assert (want > 0).float().mean() > 0.02 and torch.equal(t['depth_image_gt'], want) and not t['depth_image_gt'].requires_grad
