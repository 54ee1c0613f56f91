"""Evaluation metrics on the device (csrc/pose_eval.hip): Procrustes against the reference's own outputs (tests/golden/pose_eval.npz), known
answers, and the fused per-batch metrics of evaluate/eval.py:193-228 against an fp64 restatement written here."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ew_err

pytestmark = pytest.mark.gpu

CASES = ('rand14', 'rand17', 'rigid', 'mirror', 'collinear', 'degenerate')
J14 = [6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10]
J17 = J14 + [0, 7, 9]


def _procrustes_fp64(S1, S2):
    """fp64 restatement of utils/pose_utils.py:10-56 (SVD with the det correction), S1 / S2 [N, 3] numpy"""
    S1, S2 = np.asarray(S1, np.float64).T, np.asarray(S2, np.float64).T
    mu1, mu2 = S1.mean(1, keepdims=True), S2.mean(1, keepdims=True)
    X1, X2 = S1 - mu1, S2 - mu2
    K = X1 @ X2.T
    U, _, Vh = np.linalg.svd(K)
    Z = np.eye(3)
    Z[-1, -1] = np.sign(np.linalg.det(U @ Vh))
    R = Vh.T @ Z @ U.T
    s = np.trace(R @ K) / (X1 ** 2).sum()
    return (s * R @ S1 + (mu2 - s * R @ mu1)).T


def _rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'pose_eval.npz'))


@pytest.mark.parametrize('case', CASES)
def test_similarity_transform_matches_the_reference(dev, golden, case):
    from whmr_amd.utils.pose_utils import reconstruction_error
    S1, S2 = (torch.from_numpy(golden[case + k]).to(dev) for k in ('_S1', '_S2'))
    re, S1_hat = reconstruction_error(S1, S2, reduction=None)
    ref_hat, ref_re = golden[case + '_S1_hat'], golden[case + '_re']
    assert S1_hat.is_cuda and re.is_cuda and S1_hat.shape == S1.shape and re.shape == (S1.shape[0],)
    if case == 'degenerate':                                     # var1 = 0: NaN, as numpy
        assert torch.isnan(S1_hat).all() and torch.isnan(re).all()
        return
    assert np.abs(S1_hat.cpu().numpy() - ref_hat).max() <= 1e-5
    assert np.abs(re.cpu().numpy() - ref_re).max() <= 1e-5
    m, _ = reconstruction_error(S1, S2)
    s, _ = reconstruction_error(S1, S2, reduction='sum')
    assert abs(m.item() - ref_re.mean()) <= 1e-5 and abs(s.item() - ref_re.sum()) <= 1e-4


def test_similarity_transform_layouts(dev, golden):
    """[B, 3, N] points are columns (pose_utils.py:17-21), one-sample form, 2-D points raise, host data raises"""
    from whmr_amd.utils import pose_utils as PU
    S1, S2 = (torch.from_numpy(golden['rand17' + k]).to(dev) for k in ('_S1', '_S2'))
    ref = golden['rand17_S1_hat']
    cols = PU.compute_similarity_transform_batch(S1.transpose(1, 2), S2.transpose(1, 2))
    assert cols.shape == (8, 3, 17) and np.abs(cols.transpose(1, 2).cpu().numpy() - ref).max() <= 1e-5
    one = PU.compute_similarity_transform(S1[3], S2[3])
    assert one.shape == (17, 3) and np.abs(one.cpu().numpy() - ref[3]).max() <= 1e-5
    with pytest.raises(NotImplementedError):
        PU.compute_similarity_transform_batch(S1[..., :2], S2[..., :2])
    with pytest.raises(NotImplementedError):
        PU.reconstruction_error(S1[..., :2].transpose(1, 2), S2[..., :2].transpose(1, 2))
    with pytest.raises(RuntimeError, match='on the device'):
        PU.reconstruction_error(S1.cpu(), S2.cpu())


def test_similarity_transform_known_answers(dev):
    from whmr_amd import _lib
    rng = np.random.default_rng(7)
    B, N = 32, 17
    S1 = 0.5 * rng.standard_normal((B, N, 3))
    R = np.stack([_rotation(rng) for _ in range(B)])
    s, t = rng.uniform(0.5, 2.0, (B, 1, 1)), rng.uniform(-1, 1, (B, 1, 3))
    S2 = (s * np.einsum('bij,bnj->bni', R, S1) + t).astype(np.float32)
    S1 = S1.astype(np.float32)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    # an exact similarity: PA error ~ 0 and S1_hat = S2
    hat, err = _lib.similarity_transform(d(S1), d(S2))
    assert err.abs().max().item() <= 1e-6 and np.abs(hat.cpu().numpy() - S2).max() <= 2e-6
    # identical inputs
    hat, err = _lib.similarity_transform(d(S1), d(S1))
    assert err.abs().max().item() <= 1e-7 and np.abs(hat.cpu().numpy() - S1).max() <= 1e-6
    # a reflected target: the proper rotation of the reference, not the reflection
    M = S1 * np.array([1.0, -1.0, 1.0], np.float32) + 0.01 * rng.standard_normal(S1.shape).astype(np.float32)
    hat, err = _lib.similarity_transform(d(S1), d(M))
    ref = np.stack([_procrustes_fp64(a, b) for a, b in zip(S1, M)])
    ref_err = np.sqrt(((ref - M) ** 2).sum(-1)).mean(-1)
    assert np.abs(hat.cpu().numpy() - ref).max() <= 1e-5 and np.abs(err.cpu().numpy() - ref_err).max() <= 1e-5
    assert ref_err.min() > 0.05                                  # a reflection is not reachable by a rotation: the error stays large


# ---- fused per-batch metrics ---------------------------------------------------------------------------------------------------------------
def _meshes(assets, dev, B, seed):
    """synthetic SMPL ground truth (axis-angle pose, pose2rot=True) and a prediction perturbed from it"""
    from whmr_amd.models.smpl import SMPL
    smpl = SMPL(arrays=assets['smpl']).to(dev)
    g = torch.Generator().manual_seed(seed)
    pose = 0.3 * torch.randn(B, 72, generator=g)
    betas = torch.randn(B, 10, generator=g)
    gt = smpl(betas=betas.to(dev), body_pose=pose[:, 3:].to(dev), global_orient=pose[:, :3].to(dev), pose2rot=True).vertices
    pose_p = pose + 0.1 * torch.randn(B, 72, generator=g)
    betas_p = betas + 0.3 * torch.randn(B, 10, generator=g)
    pred = smpl(betas=betas_p.to(dev), body_pose=pose_p[:, 3:].to(dev), global_orient=pose_p[:, :3].to(dev), pose2rot=True).vertices
    pred = pred + torch.tensor([0.05, -0.02, 0.1], device=dev)   # plus a global offset that the pelvis alignment removes
    return smpl, pose, betas, pred.contiguous(), gt.contiguous()


def _jreg(seed=3):
    g = torch.Generator().manual_seed(seed)
    J = torch.rand(17, 6890, generator=g) * (torch.rand(17, 6890, generator=g) < 0.02)
    return J / J.sum(1, keepdim=True)


def _restate(pred, gt, J, jm):
    """fp64 restatement of evaluate/eval.py:193-228 (joint regression, pelvis, MPJPE, reconstruction_error, PVE)"""
    pred, gt, J = pred.double().cpu(), gt.double().cpu(), J.double().cpu()
    gk, pk = torch.matmul(J, gt), torch.matmul(J, pred)
    gk = gk[:, jm, :] - gk[:, [0], :]
    pk = pk[:, jm, :] - pk[:, [0], :]
    pve = torch.sqrt(((pred - gt) ** 2).sum(-1)).mean(-1)
    mpjpe = torch.sqrt(((pk - gk) ** 2).sum(-1)).mean(-1)
    pa = torch.from_numpy(np.stack([_procrustes_fp64(a, b) for a, b in zip(pk.numpy(), gk.numpy())]))
    pa_err = torch.sqrt(((pa - gk) ** 2).sum(-1)).mean(-1)
    return dict(mpjpe=mpjpe, pa_mpjpe=pa_err, pve=pve, pred_j=pk, pred_j_pa=pa)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs() / b.abs()).max().item()


@pytest.mark.parametrize('B', [1, 5, 64, 257])
@pytest.mark.parametrize('jm', [J14, J17], ids=['J14', 'J17'])
def test_pose_metrics_matches_the_eval_restatement(dev, assets, B, jm):
    from whmr_amd import _lib
    _, _, _, pred, gt = _meshes(assets, dev, B, seed=B)
    J = _jreg()
    nj = len(jm)
    pred_j = torch.empty(B, nj, 3, device=dev)
    pred_j_pa = torch.empty(B, nj, 3, device=dev)
    mpjpe, pa, pve = _lib.pose_metrics(pred, gt, J.to(dev), torch.tensor(jm, dtype=torch.int32, device=dev), pred_j=pred_j, pred_j_pa=pred_j_pa)
    ref = _restate(pred, gt, J, jm)
    assert ref['mpjpe'].min() > 1e-3 and ref['pa_mpjpe'].min() > 1e-4                     # the perturbation is visible in every metric
    assert _rel(mpjpe, ref['mpjpe']) < 1e-6
    assert _rel(pa, ref['pa_mpjpe']) < 1e-6
    assert _rel(pve, ref['pve']) < 1e-6
    assert ew_err(pred_j, ref['pred_j']) < 1e-6
    assert ew_err(pred_j_pa, ref['pred_j_pa']) < 1e-6


def test_pose_metrics_is_deterministic_and_graph_capturable(dev, assets):
    from whmr_amd import _lib
    B = 64
    _, _, _, pred, gt = _meshes(assets, dev, B, seed=11)
    J, jm = _jreg().to(dev), torch.tensor(J17, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.pose_metrics_workspace_bytes(B, 6890, 17), dtype=torch.uint8, device=dev)
    outs = [torch.empty(B, device=dev) for _ in range(3)] + [torch.empty(B, 17, 3, device=dev) for _ in range(2)]

    def run():
        _lib.pose_metrics(pred, gt, J, jm, *outs[:3], pred_j=outs[3], pred_j_pa=outs[4], workspace=ws)
    run()
    first = [o.clone() for o in outs]
    run()
    assert all(torch.equal(a, b) for a, b in zip(first, outs))            # bit-identical: fixed-order reductions, no atomics
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    for o in outs:
        o.fill_(-1.0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for o in outs:
        o.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, outs))


@pytest.mark.parametrize('dataset', ['3dpw', 'mpi-inf-3dhp'])
def test_pose_evaluator_over_uneven_batches(dev, assets, dataset):
    from whmr_amd.evaluate import PoseEvaluator
    from whmr_amd.models.smpl import SMPL
    J = _jreg()
    sizes = (7, 64, 30)
    ev = PoseEvaluator(J.numpy(), dataset, 128, dev)
    preds, gts = [], []
    for i, n in enumerate(sizes):
        smpl, pose, betas, pred, _ = _meshes(assets, dev, n, seed=100 + i)
        gt = ev.gt_vertices(smpl, pose.to(dev), betas.to(dev))
        ev.update(pred, gt)
        preds.append(pred)
        gts.append(gt)
    assert ev.count == sum(sizes)
    jm = J17 if dataset == 'mpi-inf-3dhp' else J14
    ref = _restate(torch.cat(preds), torch.cat(gts), J, jm)
    got = ev.per_sample()
    assert set(got) == {'mpjpe', 'recon_err', 'pve'} and all(v.shape == (sum(sizes),) for v in got.values())
    for k, r in (('mpjpe', 'mpjpe'), ('recon_err', 'pa_mpjpe'), ('pve', 'pve')):
        assert _rel(torch.from_numpy(got[k]), ref[r]) < 1e-6, k
    summ = ev.summary()
    for k, r in (('mpjpe', 'mpjpe'), ('pa-mpjpe', 'pa_mpjpe'), ('pve', 'pve')):
        assert abs(summ[k] - 1000 * ref[r].mean().item()) <= 1e-6 * 1000 * ref[r].mean().item(), k
    # 3DPW: the female rows of the ground truth come from the female model (trainer.py:786-791)
    smpl, pose, betas, _, _ = _meshes(assets, dev, 6, seed=200)
    arrays = dict(assets['smpl'])
    arrays['v_template'] = arrays['v_template'] * 1.05
    female = SMPL(arrays=arrays).to(dev)
    gender = torch.tensor([0, 1, 1, 0, 1, 0], device=dev)
    v = ev.gt_vertices(smpl, pose.to(dev), betas.to(dev), gender=gender, smpl_female=female)
    vm = ev.gt_vertices(smpl, pose.to(dev), betas.to(dev))
    vf = ev.gt_vertices(female, pose.to(dev), betas.to(dev))
    assert torch.equal(v[gender == 1], vf[gender == 1]) and torch.equal(v[gender == 0], vm[gender == 0])
    with pytest.raises(ValueError):
        ev.update(torch.zeros(30, 6890, 3, device=dev), torch.zeros(30, 6890, 3, device=dev))
