"""Writes tests/golden/one_euro.npz by driving the reference tree's OneEuroFilter (models/ViTPose/mmpose/core/post_processing/one_euro_filter.py,
imported UNMODIFIED from a checkout) the way the smoothing stage defines its scalar channel: built with fps = d_cutoff, called with t_e = the frame
gap.  The signals are strictly positive (the class's missing-keypoint mask never fires) and fp32-representable (the class stores its first sample
as float32).  The fixture holds inputs, gaps, parameters and outputs only.

    python tests/golden/make_golden_smooth.py /path/to/W-HMR
"""
import importlib.util
import os
import sys

import numpy as np

PARAMS = [(0.004, 1.0, 1.0),        # (min_cutoff, beta, d_cutoff): the defaults of demo/whmr_demo.py:135-144
          (1.7, 0.3, 30.0)]         # the class's own defaults
GAPS = [[1] * 8, [2] * 8, [3] * 8, [1, 2, 1, 3, 3, 1, 2, 1]]
N, C = 9, 14

if __name__ == '__main__':
    path = os.path.join(sys.argv[1], 'models', 'ViTPose', 'mmpose', 'core', 'post_processing', 'one_euro_filter.py')
    spec = importlib.util.spec_from_file_location('one_euro_filter', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(23)
    xs, gaps, params, outs = [], [], [], []
    for p in PARAMS:
        for g in GAPS:
            scale = 10.0 ** rng.uniform(-1, 3, size=C)                                   # channels from 0.1 (a shape coefficient) to 1000 (a focal length)
            walk = np.cumsum(rng.normal(0, 0.05, size=(N, C)), 0)
            x = ((1.0 + np.abs(walk)) * scale).astype(np.float32).astype(np.float64)
            assert (x > 0).all()
            f = mod.OneEuroFilter(x[0], min_cutoff=p[0], beta=p[1], fps=p[2])
            y = [x[0]] + [np.array(f(x[k + 1], t_e=float(g[k])), dtype=np.float64) for k in range(N - 1)]
            xs.append(x); gaps.append(g); params.append(p); outs.append(np.stack(y))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'one_euro.npz')
    np.savez_compressed(out, x=np.stack(xs), gaps=np.asarray(gaps, dtype=np.int64), params=np.asarray(params, dtype=np.float64), out=np.stack(outs))
    print(out, np.stack(xs).shape, np.stack(outs).shape)
