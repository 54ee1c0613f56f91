"""Evaluation metrics (MPJPE / PA-MPJPE / PVE): what can be checked without a device -- the golden fixture and the public API's refusal of host data."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

CASES = {'rand14': 14, 'rand17': 17, 'rigid': 14, 'mirror': 17, 'collinear': 14, 'degenerate': 14}


def test_pose_eval_fixture_loads_with_the_expected_shapes():
    path = os.path.join(GOLDEN, 'pose_eval.npz')
    assert os.path.getsize(path) < 200 * 1024
    g = np.load(path)
    for name, n in CASES.items():
        S1, S2, S1_hat, re = (g[name + k] for k in ('_S1', '_S2', '_S1_hat', '_re'))
        B = S1.shape[0]
        assert S1.shape == S2.shape == S1_hat.shape == (B, n, 3) and re.shape == (B,), name
        assert S1.dtype == S2.dtype == np.float32, name
        assert np.isnan(re).all() == (name == 'degenerate'), name
        if name != 'degenerate':                                 # the fixture's own consistency: re is the mean distance of S1_hat to S2
            assert np.allclose(np.sqrt(((S1_hat - S2) ** 2).sum(-1)).mean(-1), re, rtol=0, atol=1e-12), name


def test_pose_eval_api_exists_and_refuses_host_data():
    """the public API is there, and it keeps to the no-CPU-fallback rule (test_host_cpu.py::test_no_cpu_fallback): host tensors and numpy
    arrays raise with a message that says to keep the tensors on the device"""
    from whmr_amd import _lib
    from whmr_amd.evaluate import PoseEvaluator, joint_mapper
    from whmr_amd.utils import pose_utils as PU
    S = torch.zeros(2, 14, 3)
    for host in (S, S.numpy()):
        for fn in (PU.compute_similarity_transform_batch, PU.reconstruction_error):
            with pytest.raises(RuntimeError, match='on the device'):
                fn(host, host)
        with pytest.raises(RuntimeError, match='on the device'):
            PU.compute_similarity_transform(host[0], host[0])
    with pytest.raises(RuntimeError):
        _lib.similarity_transform(S, S)
    with pytest.raises(RuntimeError):
        _lib.pose_metrics(torch.zeros(1, 6890, 3), torch.zeros(1, 6890, 3), torch.zeros(17, 6890), torch.zeros(14, dtype=torch.int32))
    assert joint_mapper('3dpw') == [6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10]
    assert joint_mapper('mpi-inf-3dhp') == [6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10, 0, 7, 9]
    with pytest.raises(RuntimeError, match='on the device'):
        PoseEvaluator(np.zeros((17, 6890), np.float32), '3dpw', 4, 'cpu')


def test_pose_eval_source_is_built_without_packed_fp32():
    from whmr_amd import build
    assert 'pose_eval.hip' in build.NO_PACKED_FP32 or os.environ.get('WHMR_BUILD_PACKED_FP32') == '1'
    assert os.path.exists(os.path.join(ROOT, 'w-hmr_amd', 'csrc', 'pose_eval.hip'))
