"""Procrustes alignment on the device: the reference's ``utils/pose_utils.py:10-76`` names and signatures over ``whmr_similarity_transform``.

The reference loops over samples on the host with ``np.linalg.svd``; here one launch aligns the whole batch (fp64 arithmetic, one wave per sample)
and the results stay on the device.  Inputs are HIP device tensors; host tensors and numpy arrays raise (keep the tensors on the device: there is
no CPU path).  3-D points only: 2-D points raise ``NotImplementedError``.  Points are read as fp32 and the results are fp32.
"""
import torch

from .. import _lib


def _device_points(S1, S2):
    for t in (S1, S2):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError('whmr_amd.utils.pose_utils takes HIP device tensors (got %s); keep the tensors on the device -- '
                               'there is no CPU fallback' % (t.device if isinstance(t, torch.Tensor) else type(t).__name__))
    if S1.shape != S2.shape:
        raise ValueError('S1 and S2 differ in shape: %s vs %s' % (tuple(S1.shape), tuple(S2.shape)))


def _batch(S1, S2):
    """[B, N, 3] / [B, 3, N] -> contiguous fp32 [B, N, 3] and whether the points were columns.  The reference's rule per sample
    (pose_utils.py:17-21): a sample whose first dimension is neither 3 nor 2 is transposed, so [3, N] (and [3, 3]) is read as columns."""
    if S1.dim() != 3:
        raise ValueError('expected [B, N, 3] or [B, 3, N] points, got %s' % (tuple(S1.shape),))
    columns = S1.shape[1] in (2, 3)
    dim = S1.shape[1] if columns else S1.shape[2]
    if dim != 3:
        raise NotImplementedError('Procrustes of %d-D points: only 3-D points are implemented on the device' % dim)
    if columns:
        S1, S2 = S1.transpose(1, 2), S2.transpose(1, 2)
    if S1.shape[1] > 64:
        raise ValueError('at most 64 points per sample (got %d)' % S1.shape[1])
    return S1.float().contiguous(), S2.float().contiguous(), columns


def _align(S1, S2):
    _device_points(S1, S2)
    a, b, columns = _batch(S1, S2)
    S1_hat, re = _lib.similarity_transform(a, b)
    return (S1_hat.transpose(1, 2) if columns else S1_hat), re


def compute_similarity_transform(S1, S2):
    """pose_utils.py:10-56 for one sample: S1, S2 [N, 3] (or [3, N]) -> S1_hat, the similarity transform (sR, t) of S1 closest to S2."""
    _device_points(S1, S2)
    if S1.dim() != 2:
        raise ValueError('expected one sample of [N, 3] or [3, N] points, got %s' % (tuple(S1.shape),))
    return _align(S1[None], S2[None])[0][0]


def compute_similarity_transform_batch(S1, S2):
    """pose_utils.py:58-63: S1, S2 [B, N, 3] (or [B, 3, N]) -> S1_hat of the same shape."""
    return _align(S1, S2)[0]


def reconstruction_error(S1, S2, reduction='mean'):
    """pose_utils.py:65-74: Procrustes alignment, then the per-sample mean point distance.  Returns (re, S1_hat); re is the mean (default),
    the sum, or (reduction=None) the [B] per-sample errors -- all device tensors."""
    S1_hat, re = _align(S1, S2)
    if reduction == 'mean':
        re = re.mean()
    elif reduction == 'sum':
        re = re.sum()
    return re, S1_hat
