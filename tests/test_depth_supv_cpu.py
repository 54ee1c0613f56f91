"""Depth auxiliary supervision (cfg.MODEL.PyMAF.DEPTH_SUPV_ON), the parts that need no device: analytic known answers of the float64 restatement
(tests/depth_reference.py) that the device rasteriser is compared with, the model's state_dict, and the host logic of the loss."""
import contextlib

import numpy as np
import pytest
import torch

import depth_reference as DR


@contextlib.contextmanager
def flags(aux=True, depth=True):
    from whmr_amd.core.cfgs import cfg
    old = (cfg.MODEL.PyMAF.AUX_SUPV_ON, cfg.MODEL.PyMAF.DEPTH_SUPV_ON)
    cfg.MODEL.PyMAF.AUX_SUPV_ON, cfg.MODEL.PyMAF.DEPTH_SUPV_ON = aux, depth
    try:
        yield cfg
    finally:
        cfg.MODEL.PyMAF.AUX_SUPV_ON, cfg.MODEL.PyMAF.DEPTH_SUPV_ON = old


def _render(verts, faces):
    return DR.rasterize_depth(verts, faces, DR.CAM, DR.FOCAL, DR.ORIG, DR.OUT)


def test_band_width_is_the_documented_one():
    assert abs(DR.band_px(128) - 0.0614) < 5e-5


def test_tilted_triangle_gives_the_screen_interpolated_inverse_depth():
    """interior centres of a single planar face: 1 / pz = sum_i w_i / z_i with the screen barycentrics w_i"""
    verts, faces, interior, inv = DR.tilted_triangle()
    out, fid = _render(verts, faces)
    assert interior.sum() > 2000 and (fid[0][interior] == 0).all()
    assert np.abs(out[0, 0] - inv)[interior].max() < 1e-12
    assert inv[interior].max() - inv[interior].min() > 0.01                            # the tilt is visible
    assert not out[0, 0][fid[0] < 0].any()


def test_centres_within_the_band_are_covered_and_take_the_clamped_depth():
    verts, faces, (row, cols), inv = DR.edge_triangle(0.03)
    out, fid = _render(verts, faces)
    assert (fid[0, row, cols] == 0).all()
    assert np.abs(out[0, 0, row, cols] - inv).max() < 1e-12
    assert (fid[0, row - 1] < 0).all()                                                  # one row further out: 1.03 px from the edge
    # the clamp matters: the plain (unclipped) interpolation at these centres gives another value
    uv = ((20.0, row + 0.53), (100.0, row + 0.53), (60.0, 100.0))
    w = DR.screen_barycentrics(uv, cols + 0.5, np.full(cols.shape, row + 0.5))
    plain = sum(wi / (z + DR.TZ) for wi, z in zip(w, (-0.3, 0.4, 0.1)))
    assert (w[2] < 0).all() and np.abs(plain - inv).max() > 1e-8


def test_centres_beyond_the_band_are_not_covered():
    verts, faces, (row, cols), _ = DR.edge_triangle(0.10)
    out, fid = _render(verts, faces)
    assert (fid[0, row] < 0).all() and not out[0, 0, row].any()
    assert (fid[0, row + 1, cols] == 0).all()                                           # the next row is inside


@pytest.mark.parametrize('faces', [[[0, 1, 2], [3, 4, 5]], [[3, 4, 5], [0, 1, 2]]], ids=['far_first', 'near_first'])
def test_the_nearer_of_two_stacked_triangles_wins(faces):
    verts, interior = DR.stacked_triangles()
    out, fid = _render(verts, np.array(faces))
    assert (fid[0][interior] == faces.index([3, 4, 5])).all()
    assert np.abs(out[0, 0][interior] - 1.0 / (DR.TZ - 0.5)).max() < 1e-12


def test_equal_depth_goes_to_the_smaller_face_index():
    verts, interior = DR.stacked_triangles()
    same = np.concatenate([verts[:, :3], verts[:, :3]], 1)
    _, fid = _render(same, np.array([[3, 4, 5], [0, 1, 2]]))
    assert (fid[0][interior] == 0).all()


def test_a_face_behind_the_camera_is_culled():
    verts, faces = DR.behind_camera_triangle()
    scr = DR.OR.project(verts, DR.CAM, DR.OR.camera_K(DR.FOCAL, DR.ORIG), DR.FOCAL, DR.ORIG, DR.OUT)
    assert (scr[..., 2] < 0).all() and (scr[..., :2] > 0).all() and (scr[..., :2] < 128).all()      # in the image, behind the camera
    out, fid = _render(verts, faces)
    assert (fid < 0).all() and not out.any()


def test_a_degenerate_face_is_skipped():
    verts, faces = DR.degenerate_triangle()
    out, fid = _render(verts, faces)
    assert (fid < 0).all() and not out.any()


def test_margin_marks_the_decided_pixels():
    verts, faces, (row, cols), _ = DR.edge_triangle(0.03)
    _, fid, margin = DR.rasterize_depth(verts, faces, DR.CAM, DR.FOCAL, DR.ORIG, DR.OUT, want_margin=True)
    assert np.allclose(margin[0, row, cols], DR.band_px(128) - 0.03, atol=1e-9)
    assert margin[0].min() > 1e-3                                                       # every pixel of this scene is decided


# ---- model state -------------------------------------------------------------------------------------------------------------------------------
def _keys(assets, aux, depth):
    from whmr_amd.models import whmr_net
    with flags(aux, depth):
        m = whmr_net(None, assets=assets, numerics='fp32')
    return m, {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_state_dict_gains_exactly_the_two_depth_head_keys(assets):
    m_off, off = _keys(assets, True, False)
    m_on, on = _keys(assets, True, True)
    assert not hasattr(m_off, 'dpth_head') and not any(k.startswith('dpth_head') for k in off)
    extra = {k: s for k, s in on.items() if k not in off}
    assert extra == {'dpth_head.predict_depth.weight': (1, 256, 3, 3), 'dpth_head.predict_depth.bias': (1,)}
    assert {k: s for k, s in on.items() if k in off} == off
    # a checkpoint trained with the flag on loads strictly (and does not without the head)
    sd = {k: v.clone() for k, v in m_on.state_dict().items()}
    sd['dpth_head.predict_depth.weight'].fill_(0.25)
    m_on.load_state_dict(sd, strict=True)
    assert (m_on.dpth_head.predict_depth.weight == 0.25).all()
    with pytest.raises(RuntimeError):
        m_off.load_state_dict(sd, strict=True)
    # torch's Conv2d initialisation: kaiming_uniform(a = sqrt(5)) -> |w| <= 1 / sqrt(fan_in), the bias likewise
    from whmr_amd.models.whmr import Depth_predict_layer
    w = Depth_predict_layer(feat_dim=256, final_cov_k=3)
    bound = 1.0 / np.sqrt(256 * 9)
    assert w.predict_depth.weight.abs().max() <= bound and w.predict_depth.weight.abs().max() > 0.5 * bound
    assert w.predict_depth.bias.abs().max() <= bound
    assert w.predict_depth.padding == (1, 1) and w.predict_depth.stride == (1, 1)


# ---- host logic ----------------------------------------------------------------------------------------------------------------------------------
def test_compute_losses_rejects_depth_without_aux():
    from whmr_amd.train import compute_losses
    with flags(aux=False, depth=True):
        with pytest.raises(ValueError) as e:
            compute_losses({'smpl_out': [None] * 4}, {})
    assert 'DEPTH_SUPV_ON' in str(e.value) and 'AUX_SUPV_ON' in str(e.value)


@pytest.mark.parametrize('valid', [(1, 0, 1), (0, 0, 0), None], ids=['one_invalid', 'all_invalid', 'none'])
def test_depth_losses_equals_the_float64_formula(valid):
    from whmr_amd.core.cfgs import cfg
    from whmr_amd.train.aux_supervision import depth_losses
    g = torch.Generator().manual_seed(3)
    pred = (torch.randn(3, 1, 13, 11, generator=g) * 1.5).requires_grad_(True)         # both sides of the smooth-L1 knee
    gt = torch.rand(3, 1, 13, 19, generator=g)[:, :, :, 4:-4] * 0.3
    vf = None if valid is None else torch.tensor(valid, dtype=torch.bool)
    w = float(cfg.LOSS.POINT_REGRESSION_WEIGHTS)
    assert w > 0
    loss = depth_losses(pred, gt, vf)
    ref, gref = DR.depth_loss(pred.detach().numpy(), gt.numpy(), valid, w)
    assert ((pred.detach() - gt).abs() > 1).any() and ((pred.detach() - gt).abs() < 1).any()
    if valid is not None and not any(valid):
        assert loss.item() == 0.0 and ref == 0.0
    else:
        assert abs(loss.item() - ref) <= 2e-6 * abs(ref)
    loss.backward()
    assert np.abs(pred.grad.numpy() - gref).max() <= 1e-6 * max(np.abs(gref).max(), 1e-30)
    # the float tensor form of the mask (has_smpl as the batch carries it) gives the same
    if valid is not None:
        assert depth_losses(pred.detach(), gt, torch.tensor(valid, dtype=torch.float32)).item() == loss.item()


def test_depth_losses_is_zero_without_a_positive_weight():
    from whmr_amd.core.cfgs import cfg
    from whmr_amd.train.aux_supervision import depth_losses
    old = cfg.LOSS.POINT_REGRESSION_WEIGHTS
    cfg.LOSS.POINT_REGRESSION_WEIGHTS = 0.0
    try:
        assert depth_losses(torch.ones(2, 1, 4, 4), torch.zeros(2, 1, 4, 4), None).item() == 0.0
    finally:
        cfg.LOSS.POINT_REGRESSION_WEIGHTS = old


def test_depth_head_output_stands_in_for_the_nchw_map():
    """DepthHeadOutput: shape without materialising, torch functions and operators on the lazily created [B, 1, H, W] fp32 view, gradients reach nhwc"""
    import torch.nn.functional as F
    from whmr_amd.train.aux_supervision import DepthHeadOutput
    y = torch.randn(2, 5, 4, 91, requires_grad=True)
    d = DepthHeadOutput(y, 90)
    assert d.shape == (2, 1, 5, 4) and d.size(1) == 1 and d.dim() == 4 and d._map is None
    gt = torch.zeros(2, 1, 5, 4)
    a = F.smooth_l1_loss(d, gt, reduction='sum')
    b = F.smooth_l1_loss(y[..., 90:].permute(0, 3, 1, 2), gt, reduction='sum')
    assert d._map is not None and a.item() == b.item()
    assert torch.equal((d * 2.0 - gt).detach(), (2.0 * d).detach()) and torch.equal((gt - d).detach(), (-d).detach())
    assert torch.equal(d.sum().detach(), y[..., 90].sum().detach()) and torch.equal(d[:, 0].detach(), y[..., 90].detach())
    a.backward()
    assert y.grad[..., :90].abs().max() == 0 and y.grad[..., 90].abs().max() > 0


def test_renderer_constructor_checks():
    from whmr_amd.utils.renderer import Depth_Renderer
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]])
    r = Depth_Renderer(orig_size=(256, 256), output_size=(128, 128), faces=faces)
    assert r.K == DR.OR.camera_K(1000.0, (256, 256)) and r.faces.dtype == torch.int32 and r.num_verts == 4
    with pytest.raises(AssertionError):
        Depth_Renderer(orig_size=(256, 256), output_size=(128, 96), faces=faces)
    with pytest.raises(RuntimeError):
        r.verts2depthimg(torch.zeros(1, 4, 3), torch.ones(1, 3))                       # host tensors
