"""Generate tests/golden/pose_eval.npz by importing the reference's utils/pose_utils.py UNMODIFIED (pure numpy) -- build container only.

Usage (from the repo root):
    python tests/golden/make_golden_eval.py /path/to/W-HMR          # a checkout of the reference (yw0208/W-HMR)

Every case holds fp32 points S1, S2 [B, N, 3] and what the reference's ``reconstruction_error(S1, S2, reduction=None)`` returns for them
(evaluated in float64 on the fp32 values): the per-sample error ``re`` [B] and ``S1_hat`` [B, N, 3].  Cases:
  rand14 / rand17  unit-scale random joints with a noisy target (the eval.py shapes, J14 and J17)
  rigid            large rotations with scale and offset (S2 = s R S1 + t + small noise)
  mirror           reflected targets (x -> -x): the det(U V^T) < 0 correction of the SVD solution
  collinear        S1 on a line (K of rank 1: R is not unique, S1_hat is)
  degenerate       all S1 points equal (var1 = 0): NaN, as numpy
Nothing from the reference is copied; the fixture is plain arrays.
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def cases(seed=0):
    rng = np.random.default_rng(seed)
    out = {}
    for n in (14, 17):
        S1 = 0.5 * rng.standard_normal((8, n, 3))
        out['rand%d' % n] = (S1, S1 + 0.05 * rng.standard_normal(S1.shape))
    S1 = 0.5 * rng.standard_normal((8, 14, 3))
    R, s, t = _rotations(rng, 8), rng.uniform(0.5, 2.0, (8, 1, 1)), rng.uniform(-1.0, 1.0, (8, 1, 3))
    out['rigid'] = (S1, s * np.einsum('bij,bnj->bni', R, S1) + t + 0.01 * rng.standard_normal(S1.shape))
    S1 = 0.5 * rng.standard_normal((6, 17, 3))
    out['mirror'] = (S1, S1 * np.array([-1.0, 1.0, 1.0]) + 0.02 * rng.standard_normal(S1.shape))
    d = rng.standard_normal((4, 1, 3))
    S1 = rng.standard_normal((4, 14, 1)) * d / np.linalg.norm(d, axis=-1, keepdims=True) + 0.3
    out['collinear'] = (S1, 0.5 * rng.standard_normal((4, 14, 3)))
    S1 = np.repeat(rng.standard_normal((2, 1, 3)), 14, axis=1)
    out['degenerate'] = (S1, 0.5 * rng.standard_normal((2, 14, 3)))
    return {k: (a.astype(np.float32), b.astype(np.float32)) for k, (a, b) in out.items()}


def main(ref):
    spec = importlib.util.spec_from_file_location('ref_pose_utils', os.path.join(ref, 'utils', 'pose_utils.py'))
    pu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pu)
    arrays = {}
    for name, (S1, S2) in cases().items():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)            # the var1 = 0 case divides 0 by 0, as intended
            re, S1_hat = pu.reconstruction_error(S1.astype(np.float64), S2.astype(np.float64), reduction=None)
        arrays.update({name + '_S1': S1, name + '_S2': S2, name + '_S1_hat': S1_hat, name + '_re': re})
        print('%-10s B=%d N=%d  re %s' % (name, S1.shape[0], S1.shape[1], np.array2string(re, precision=4)))
    path = os.path.join(HERE, 'pose_eval.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
