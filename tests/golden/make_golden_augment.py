"""Generate tests/golden/augment.npz by importing the reference's utils/imutils.py, core/constants.py and datasets/base_dataset.py UNMODIFIED --
build container only.

Usage (from the repo root):
    python tests/golden/make_golden_augment.py /path/to/W-HMR          # a checkout of the reference (yw0208/W-HMR)

Stub recipe of make_golden.py (yacs from there; cv2, skimage, albumentations, pare, joblib, torchvision as empty stand-ins): ``cv2.Rodrigues`` is
scipy's Rotation, ``cv2.imread`` hands out the synthetic images, ``skimage.transform.rotate`` is absent (the image is recorded for rot = 0 only).
BaseDataset is subclassed WITHOUT running its __init__ (it loads annotation files and SMPL): the subclass sets the attributes __init__ would have
set from the synthetic annotation arrays; every recorded number comes from the reference's own methods:
  img_*     BaseDataset.rgb_processing (is_train False: no ColorJitter; no occluders) for the rot = 0 parameter sets (kp_is_smpl False), stored as the uint8 value
            v of its float32 output v / 255 (checked to be exact) and only columns 32 .. 223, the ones the model reads
  lab_*     BaseDataset.__getitem__ for every parameter set, with augm_params replaced by the set and rgb_processing by a blank
  draw_*    BaseDataset.augm_params, 64 calls after np.random.seed(SEED)
  mask      the meta_mask of 64 __getitem__ calls after np.random.seed(SEED + 1) (augm_params replaced: the mask draws are the only ones)
  perm_*    the flip permutations of core/constants.py
Nothing from the reference is copied; the fixture is plain arrays.
"""
import os
import sys
import types

import numpy as np
import torch
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
SEED = 20240
N_DRAW = 64


def synthetic_images():
    """3 RGB images of different sizes: smooth structure + noise, a saturated flat patch"""
    rng = np.random.default_rng(7)
    out = []
    for (h, w) in ((200, 168), (150, 230), (300, 280)):
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        img = np.stack([128 + 90 * np.sin(x / 17.0 + c) * np.cos(y / (11.0 + 3 * c)) + 25 * np.sin((x + 2 * y) / 5.0) for c in range(3)], -1)
        img += rng.normal(0, 4, img.shape)
        img[h // 3:h // 3 + 40, w // 4:w // 4 + 50] = 255                     # saturated, flat
        img[h // 2:h // 2 + 12, w // 2:w // 2 + 30] = 0
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out


def synthetic_labels(shapes):
    """6 samples, two per image; sample 2's box leaves its image on two sides; sample 5 is a large (down-sampled) box"""
    rng = np.random.default_rng(11)
    n = 6
    img_of = np.array([0, 1, 2, 0, 1, 2])
    wh = np.array([[shapes[i][1], shapes[i][0]] for i in img_of], dtype=np.float64)
    center = wh * rng.uniform(0.35, 0.65, (n, 2))
    scale = np.array([0.62, 0.55, 0.9, 0.48, 0.71, 1.42])
    center[2] = [shapes[2][1] - 30.5, 41.25]                                  # top right corner: the box leaves the image on two sides
    kp = lambda k: np.concatenate([wh[:, None] * rng.uniform(0.05, 0.95, (n, k, 2)), (rng.uniform(0, 1, (n, k, 1)) > 0.25) * rng.uniform(0.2, 1, (n, k, 1))], -1)
    pose = rng.normal(0, 0.4, (n, 72))
    pose[0, :3] = [3.1, 0.05, -0.02]                                          # root turned by almost pi
    pose[1, :3] = [0.0, 0.0, 0.0]
    return {'img_of': img_of, 'center': center, 'scale': scale, 'pose': pose, 'shape': rng.normal(0, 1, (n, 10)),
            'has_smpl': np.array([1, 1, 0, 1, 1, 1], dtype=np.float32), 'part': kp(24), 'openpose': kp(25), 'smpl_2dkps': kp(24),
            'S': np.concatenate([rng.normal(0, 0.4, (n, 24, 3)), (rng.uniform(0, 1, (n, 24, 1)) > 0.2).astype(np.float64)], -1),
            'gender': np.array(['m', 'f', 'f', 'm', 'n', 'm'])}


def parameter_sets():
    """(sample, flip, rot, sc, pn, kp_is_smpl): rot in {0, +-17.3, 60}, both flips, sc in {0.75, 1, 1.25}, pn at both ends of [0.6, 1.4]"""
    sets, i = [], 0
    pns = ([0.6, 1.4, 1.0], [1.4, 0.6, 1.4], [1.0, 1.0, 1.0], [0.6, 0.6, 1.4])
    for rot in (0.0, 17.3, 0.0, -17.3, 0.0, 60.0):
        for flip in (0, 1):
            sets.append((i % 6, flip, rot, (0.75, 1.0, 1.25)[i % 3], pns[i % 4], False))
            i += 1
    sets.append((3, 1, 0.0, 1.25, pns[1], True))
    sets.append((4, 1, 60.0, 1.0, pns[0], True))
    return sets


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install_stubs(ref, images):
    from make_golden import CfgNode                                           # the yacs stand-in of make_golden.py

    def rodrigues(x):
        x = np.asarray(x, dtype=np.float64)
        if x.size == 3:
            return Rotation.from_rotvec(x.reshape(3)).as_matrix(), None
        return Rotation.from_matrix(x).as_rotvec().reshape(3, 1), None
    _mod('yacs')
    _mod('yacs.config', CfgNode=CfgNode)
    _mod('cv2', Rodrigues=rodrigues, imread=lambda name: images[int(os.path.basename(name))][:, :, ::-1])
    _mod('joblib')
    _mod('skimage')
    _mod('skimage.transform')
    _mod('albumentations', Compose=lambda transforms: (lambda image: {'image': image}), ColorJitter=lambda **k: None)
    _mod('pare')
    _mod('pare.dataset')
    _mod('pare.dataset.coco_occlusion', load_coco_occluders=None, load_pascal_occluders=None, occlude_with_coco_objects=None,
         occlude_with_pascal_objects=None)
    _mod('pare.utils')
    _mod('pare.utils.image_utils', random_crop=None)
    _mod('pare.models', SMPL=None)
    _mod('torchvision')
    _mod('torchvision.transforms', Normalize=lambda mean, std: (lambda t: t))
    for pkg in ('datasets', 'utils'):                                         # the reference's packages without their __init__ (they import everything)
        _mod(pkg).__path__ = [os.path.join(ref, pkg)]
    sys.path.insert(0, ref)
    if not hasattr(np, 'float'):
        np.float = float                                                     # base_dataset.py:76 (numpy < 1.24 spelling), not reached here


def main(ref):
    images = synthetic_images()
    lab = synthetic_labels([im.shape[:2] for im in images])
    install_stubs(ref, images)
    from core.cfgs import cfg
    cfg.merge_from_file(os.path.join(ref, 'configs/pymaf_config.yaml'))
    from core import constants, path_config
    if not hasattr(path_config, 'PASCAL_ROOT'):
        path_config.PASCAL_ROOT = ''                                         # base_dataset.py:21 imports a name its path_config does not define
    from datasets.base_dataset import BaseDataset

    class Stand(BaseDataset):
        def __init__(self, is_train, dataset='synthetic'):
            self.dataset, self.is_train, self.occluders = dataset, is_train, None
            self.options = types.SimpleNamespace(noise_factor=0.4, rot_factor=30, scale_factor=0.25, USE_SYNTHETIC_OCCLUSION=False)
            self.img_dir, self.imgname = '', [str(i) for i in lab['img_of']]
            self.normalize_img = lambda t: t
            self.scale, self.center = lab['scale'], lab['center']
            self.pose, self.betas, self.has_smpl = lab['pose'].astype(float), lab['shape'].astype(float), lab['has_smpl']
            self.smpl_2dkps, self.has_smpl_2dkps = lab['smpl_2dkps'], 1
            self.pose_3d, self.has_pose_3d = lab['S'], 1
            self.keypoints = np.concatenate([lab['openpose'], lab['part']], axis=1)
            self.gender = np.array([0 if str(g) == 'm' else 1 for g in lab['gender']]).astype(np.int32)

    class Preset(Stand):
        params = None

        def augm_params(self):
            return self.params

        def rgb_processing(self, rgb_img, center, scale, rot, flip, pn):
            return np.zeros((3, 256, 256), dtype=np.float32)

    out = {'perm_smpl_joints': np.array(constants.SMPL_JOINTS_FLIP_PERM), 'perm_j24': np.array(constants.J24_FLIP_PERM),
           'perm_j49': np.array(constants.J49_FLIP_PERM), 'perm_smpl_j49': np.array(constants.SMPL_J49_FLIP_PERM),
           'perm_smpl_pose': np.array(constants.SMPL_POSE_FLIP_PERM)}
    for i, im in enumerate(images):
        out['image%d' % i] = im
    for k, v in lab.items():
        out['ann_' + k] = v

    sets = parameter_sets()
    out['set_sample'] = np.array([s[0] for s in sets])
    out['set_flip'] = np.array([s[1] for s in sets])
    out['set_rot'] = np.array([s[2] for s in sets])
    out['set_sc'] = np.array([s[3] for s in sets])
    out['set_pn'] = np.array([s[4] for s in sets])
    out['set_is_smpl'] = np.array([s[5] for s in sets])
    keys = ('pose', 'betas', 'smpl_2dkps', 'pose_3d', 'keypoints', 'keypoints_world', 'has_smpl', 'has_pose_3d', 'scale', 'center', 'orig_shape',
            'is_flipped', 'rot_angle', 'gender', 'sample_index', 'bbox_height', 'bbox_width', 'focal', 'bbox_info')
    rows = {k: [] for k in keys}
    plain = Stand(is_train=False)
    for n, (idx, flip, rot, sc, pn, is_smpl) in enumerate(sets):
        ds = Preset(is_train=True, dataset='surreal' if is_smpl else 'synthetic')
        ds.params = (flip, np.array(pn), rot, sc)
        item = ds[idx]
        for k in keys:
            rows[k].append(np.asarray(item[k]))
        if rot == 0 and not is_smpl:
            img = images[lab['img_of'][idx]].astype(np.float32)
            rgb = BaseDataset.rgb_processing(plain, img, lab['center'][idx].copy(), sc * lab['scale'][idx], 0, flip, np.array(pn))
            u8 = np.rint(rgb * 255.0).astype(np.uint8)
            assert rgb.dtype == np.float32 and rgb.shape == (3, 256, 256) and np.array_equal(u8.astype(np.float32) / 255.0, rgb)
            out['img_%d' % n] = np.ascontiguousarray(u8.transpose(1, 2, 0)[:, 32:224])
    for k in keys:
        out['lab_' + k] = np.stack(rows[k])

    np.random.seed(SEED)
    drawer = Stand(is_train=True)
    draws = [drawer.augm_params() for _ in range(N_DRAW)]
    out['draw_flip'] = np.array([d[0] for d in draws])
    out['draw_pn'] = np.stack([d[1] for d in draws])
    out['draw_rot'] = np.array([float(d[2]) for d in draws])
    out['draw_sc'] = np.array([float(d[3]) for d in draws])
    np.random.seed(SEED + 1)
    ds = Preset(is_train=True)
    ds.params = (0, np.ones(3), 0, 1)
    out['mask'] = np.stack([ds[i % 6]['meta_mask'].numpy() for i in range(N_DRAW)]).astype(np.uint8)
    out['seed'] = np.array(SEED)

    # the restatement must reproduce what was just recorded (tests/test_augment_cpu.py asserts the same from the file)
    import augment_reference as AR
    for n, (idx, flip, rot, sc, pn, is_smpl) in enumerate(sets):
        if 'img_%d' % n in out:
            mine = AR.rgb_patch(images[lab['img_of'][idx]], lab['center'][idx], sc * lab['scale'][idx], 0, flip, pn)[:, 32:224]
            d = np.abs(mine.astype(int) - out['img_%d' % n].astype(int))
            print('set %2d  image: max grey-level difference %d, differing pixels %.4f %%' % (n, d.max(), 100.0 * (d > 0).mean()))
    path = os.path.join(HERE, 'augment.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
