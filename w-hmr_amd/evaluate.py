"""3D pose evaluation on the device: the metric half of evaluate/eval.py:130-330 and Trainer.validate (core/trainer.py:754-907).

    ev = PoseEvaluator(J_regressor_h36m, dataset_name, len(dataset), device)
    for batch in loader:
        gt_verts = ev.gt_vertices(smpl, gt_pose, gt_betas)                 # or (..., gender, smpl_female) for 3DPW, trainer.py:786-791
        ev.update(pred_vertices, gt_verts)                                  # no host sync
    print(ev.summary())                                                     # {'mpjpe', 'pa-mpjpe', 'pve'} in mm: the only host sync

Per batch the reference regresses the H36M joints, subtracts the pelvis, and then leaves the device twice (``.cpu().numpy()``) for a host loop
of ``np.linalg.svd`` Procrustes calls.  Here that is ``whmr_pose_metrics``: two launches per batch, results written straight into device arrays at
the running sample offset.
"""
import torch

from . import _lib
from .core.constants import H36M_TO_J14, H36M_TO_J17


def joint_mapper(dataset_name):
    """H36M regressor rows scored for a dataset (eval.py:150, trainer.py:766): J17 for MPI-INF-3DHP, J14 otherwise."""
    return H36M_TO_J17 if dataset_name == 'mpi-inf-3dhp' else H36M_TO_J14


class PoseEvaluator:
    """MPJPE, PA-MPJPE and PVE of every sample, accumulated on the device.  J_regressor: the dense [17, 6890] H36M regressor (array or tensor);
    dataset_name picks the joint map as eval.py:150 does (J17 for 'mpi-inf-3dhp', J14 otherwise); num_samples: the capacity."""

    def __init__(self, J_regressor, dataset_name, num_samples, device):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('PoseEvaluator scores on a HIP device (got %s); keep the tensors on the device -- there is no CPU fallback' % self.device)
        self.J_regressor = torch.as_tensor(J_regressor, dtype=torch.float32).to(self.device).contiguous()
        self.joint_mapper = joint_mapper(dataset_name)
        self._map = torch.tensor(self.joint_mapper, dtype=torch.int32, device=self.device)
        self.num_samples = int(num_samples)
        self.mpjpe = torch.zeros(self.num_samples, dtype=torch.float32, device=self.device)
        self.recon_err = torch.zeros_like(self.mpjpe)
        self.pve = torch.zeros_like(self.mpjpe)
        self.count = 0
        self._ws = None

    def gt_vertices(self, smpl, gt_pose, gt_betas, gender=None, smpl_female=None):
        """Ground-truth mesh from axis-angle pose [B, 72] and betas (eval.py:178,194; trainer.py:778-791).  With ``gender``, ``smpl`` is the male
        model and the rows with gender == 1 come from ``smpl_female``."""
        def run(m):
            return m(betas=gt_betas, body_pose=gt_pose[:, 3:], global_orient=gt_pose[:, :3], pose2rot=True).vertices
        verts = run(smpl)
        if gender is not None:
            female = (gender == 1).view(-1, 1, 1)
            verts = torch.where(female, run(smpl_female), verts)
        return verts

    def update(self, pred_vertices, gt_vertices):
        """Score one batch ([B, 6890, 3] each, metres) into rows [count, count + B).  Returns this batch's (mpjpe, pa_mpjpe, pve) views."""
        _lib._dev(pred_vertices, gt_vertices)
        B, V = pred_vertices.shape[:2]
        if self.count + B > self.num_samples:
            raise ValueError('PoseEvaluator holds %d samples; %d + %d do not fit' % (self.num_samples, self.count, B))
        need = _lib.pose_metrics_workspace_bytes(B, V, len(self.joint_mapper))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        rows = slice(self.count, self.count + B)
        out = (self.mpjpe[rows], self.recon_err[rows], self.pve[rows])
        _lib.pose_metrics(pred_vertices.float().contiguous(), gt_vertices.float().contiguous(), self.J_regressor, self._map, *out,
                          workspace=self._ws)
        self.count += B
        return out

    def per_sample(self):
        """numpy arrays of the samples scored so far, in metres, as eval.py stores them: {'mpjpe', 'recon_err', 'pve'}."""
        n = self.count
        return {k: getattr(self, k)[:n].cpu().numpy() for k in ('mpjpe', 'recon_err', 'pve')}

    def summary(self):
        """Means over the samples scored so far in mm (x1000: eval.py:328-330, trainer.py:884-887).  The one host sync."""
        n = self.count
        m = torch.stack([self.mpjpe[:n].double().mean(), self.recon_err[:n].double().mean(), self.pve[:n].double().mean()]).cpu()
        return {'mpjpe': 1000 * m[0].item(), 'pa-mpjpe': 1000 * m[1].item(), 'pve': 1000 * m[2].item()}
