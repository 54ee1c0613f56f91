"""The MXFP8 pilot on the host: it is a switch of the bf16 ViT inference path, off by default and not a numerics mode."""
import pytest


def test_mx_pilot_is_off_by_default_and_not_a_numerics_mode(monkeypatch):
    from whmr_amd.models.pose_vit import ViT
    monkeypatch.delenv('WHMR_MX_PILOT', raising=False)
    assert ViT(numerics='bf16').mx_pilot is False
    for bad in ('mxfp8', 'fp8'):
        with pytest.raises(AssertionError):
            ViT(numerics=bad)
    monkeypatch.setenv('WHMR_MX_PILOT', '1')
    m = ViT(numerics='bf16')
    assert m.mx_pilot is True and m.numerics == 'bf16'


def test_mx_pilot_does_not_change_the_training_graph(monkeypatch):
    """the pilot only touches the eval forward: the training autograd of a ViT with the pilot on picks the bf16 operands and the bf16 attention
    backward exactly as without it"""
    from whmr_amd.models.pose_vit import ViT
    from whmr_amd.train import vit_autograd as VA
    monkeypatch.setenv('WHMR_MX_PILOT', '1')
    on = ViT(img_size=(256, 192), numerics='bf16')
    monkeypatch.setenv('WHMR_MX_PILOT', '0')
    off = ViT(img_size=(256, 192), numerics='bf16')
    assert on.mx_pilot and not off.mx_pilot
    assert VA._dt(on) == VA._dt(off)
    for N in (192, 196):
        assert VA._hip_attention_bwd(on, N) == VA._hip_attention_bwd(off, N)


def test_mx_entry_points_are_bound():
    from whmr_amd import _lib as L
    for fn in ('gemm_blk_mx', 'quantize_mx', 'layernorm_blk_mx'):
        assert callable(getattr(L, fn))
