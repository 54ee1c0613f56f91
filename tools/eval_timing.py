"""Per-batch scoring cost: whmr_pose_metrics (two launches, HIP events over 50 calls) vs the reference's host path as evaluate/eval.py:193-228 runs it
-- torch matmul joint regression on the device, .cpu(), then one numpy SVD Procrustes per sample (restated here) -- at B = 64 and 1024, J14."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from whmr_amd import _lib
from whmr_amd.core.constants import H36M_TO_J14

dev = torch.device('cuda:0')


def procrustes_host(S1, S2):
    """the SVD solution with the det correction, one sample [N, 3], numpy (utils/pose_utils.py:10-56 restated)"""
    S1, S2 = S1.T, S2.T
    mu1, mu2 = S1.mean(1, keepdims=True), S2.mean(1, keepdims=True)
    X1, X2 = S1 - mu1, S2 - mu2
    K = X1 @ X2.T
    U, _, Vh = np.linalg.svd(K)
    Z = np.eye(3)
    Z[-1, -1] = np.sign(np.linalg.det(U @ Vh))
    R = Vh.T @ Z @ U.T
    s = np.trace(R @ K) / (X1 ** 2).sum()
    return (s * R @ S1 + (mu2 - s * R @ mu1)).T


def host_path(pred, gt, J, jm):
    gk, pk = torch.matmul(J, gt), torch.matmul(J, pred)
    gk = gk[:, jm, :] - gk[:, [0], :]
    pk = pk[:, jm, :] - pk[:, [0], :]
    pve = torch.sqrt(((pred - gt) ** 2).sum(-1)).mean(-1).cpu().numpy()
    mpjpe = torch.sqrt(((pk - gk) ** 2).sum(-1)).mean(-1).cpu().numpy()
    p, g = pk.cpu().numpy(), gk.cpu().numpy()
    hat = np.stack([procrustes_host(a, b) for a, b in zip(p, g)])
    return mpjpe, np.sqrt(((hat - g) ** 2).sum(-1)).mean(-1), pve


gen = torch.Generator().manual_seed(0)
J = torch.rand(17, 6890, generator=gen) * (torch.rand(17, 6890, generator=gen) < 0.02)
J = (J / J.sum(1, keepdim=True)).to(dev)
jm = torch.tensor(H36M_TO_J14, dtype=torch.int32, device=dev)
print('torch %s, host threads %d' % (torch.__version__, torch.get_num_threads()))
for B in (64, 1024):
    gt = torch.randn(B, 6890, 3, generator=gen).to(dev)
    pred = gt + 0.02 * torch.randn(B, 6890, 3, generator=gen).to(dev)
    ws = torch.empty(_lib.pose_metrics_workspace_bytes(B, 6890, 14), dtype=torch.uint8, device=dev)
    outs = [torch.empty(B, device=dev) for _ in range(3)]
    fn = lambda: _lib.pose_metrics(pred, gt, J, jm, *outs, workspace=ws)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    reps = 50
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    dev_us = e0.elapsed_time(e1) / reps * 1e3
    ref = host_path(pred, gt, J, H36M_TO_J14)                 # warm-up + the values to compare
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        host_path(pred, gt, J, H36M_TO_J14)
        t.append(time.perf_counter() - t0)
    err = max(np.abs(o.cpu().numpy() - r).max() / np.abs(r).max() for o, r in zip(outs, ref))
    byt = 2 * B * 6890 * 3 * 4
    print('B %4d: whmr_pose_metrics %.1f us (%.2f MB of vertices -> %.0f GB/s) | host path (matmul + .cpu() + numpy SVD loop) median %.2f ms, '
          'min %.2f ms | max rel. difference %.1e' % (B, dev_us, byt / 1e6, byt / dev_us / 1e3, 1e3 * np.median(t), 1e3 * min(t), err), flush=True)
