"""Writes tests/golden/skeleton.npz from the reference tree's datasets/data_utils/kp_utils.py, imported UNMODIFIED from a checkout (it needs numpy
only): the 25 bones of get_spin_skeleton() and the 49 joint names of get_spin_joint_names(), which core/constants.py restates as SPIN_SKELETON and
from which it takes the left / right / centre class of every bone.  The fixture holds the bone table and the names only.

    python tests/golden/make_golden_skeleton.py /path/to/W-HMR
"""
import importlib.util
import os
import sys

import numpy as np

if __name__ == '__main__':
    path = os.path.join(sys.argv[1], 'datasets', 'data_utils', 'kp_utils.py')
    spec = importlib.util.spec_from_file_location('kp_utils', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bones = np.asarray(mod.get_spin_skeleton(), dtype=np.int32)
    names = np.asarray(mod.get_spin_joint_names())
    assert bones.shape == (25, 2) and names.shape == (49,) and names.dtype.kind == 'U'
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'skeleton.npz')
    np.savez_compressed(out, bones=bones, names=names)
    print(out, bones.shape, names.shape)
