"""Training batches on the device: the sample-making of ``BaseDataset.__getitem__`` (datasets/base_dataset.py:249-384) for a whole batch behind
one call, producing the dictionary ``core/trainer.py:383-403`` reads.

The reference makes every sample on the CPU: it draws the augmentation (``augm_params``), cuts / rotates the person box (utils/imutils.py:crop),
resizes it with Pillow, flips it, scales the colour channels, normalises, and pushes keypoints, 3-D joints and the SMPL pose through the same flip /
rotation / scale.  Here the annotation arrays are uploaded once (``TrainBatchMaker``), and per batch the host computes -- in float64 numpy, exactly as
the reference does -- only the per-sample geometry (box corners and pad with their ``int`` truncations, the 3 x 3 ``get_transform`` matrix, the
rotation's inverse map) and uploads it as ONE table (struct whmr_augment_item, include/whmr_hip.h) that also names every source image by pointer,
size and row stride.  Everything per pixel and per label runs in csrc/augment.hip (five launches, no host synchronisation).

Out of scope (the image differs from the reference's where these are switched on): the synthetic occluders (``USE_SYNTHETIC_OCCLUSION``: needs the
Pascal VOC objects), the albumentations ``ColorJitter`` (p = 0.2; its arithmetic and random order are not pinned here) and ``agora_crop``'s special
case (no crop).  A sample whose crop raises in the reference (base_dataset.py:282-287 then retries with the unscaled box) raises here.
Image decoding stays with the caller.
"""
import struct

import numpy as np
import torch

from .. import _lib as L
from .img_utils import MEAN, STD

RES = 256
X_SLICE = (32, 224)
N_MASK = 431


def draw_augm_params(n, rot_factor=30, noise_factor=0.4, scale_factor=0.25, is_train=True, rng=np.random):
    """``augm_params`` (base_dataset.py:151-181) for n samples -> flip [n] int64, pn [n, 3], rot [n], sc [n] (float64).  Same distributions and the
    same sequence of draws per sample, the two discarded ``randn`` behind ``uniform() > 0.7`` included: the same seed gives the same numbers."""
    flip, pn, rot, sc = np.zeros(n, dtype=np.int64), np.ones((n, 3)), np.zeros(n), np.ones(n)
    if is_train:
        for i in range(n):
            if rng.uniform() <= 0.5:
                flip[i] = 1
            pn[i] = rng.uniform(1 - noise_factor, 1 + noise_factor, 3)
            if rng.uniform() > 0.6:
                rot[i] = min(2 * rot_factor, max(-2 * rot_factor, rng.randn() * rot_factor))
            sc[i] = min(1 + scale_factor, max(1 - scale_factor, rng.randn() * scale_factor + 1))
            if rng.uniform() > 0.7:
                rng.randn()
                rng.randn()
    return flip, pn, rot, sc


def draw_meta_mask(n, rng=np.random, is_train=True, percent=0.3):
    """the vertex mask of base_dataset.py:344-353 for n samples -> [n, 431] uint8 (1 = kept)"""
    mask = np.ones((n, N_MASK), dtype=np.uint8)
    if is_train:
        for i in range(n):
            masked = int(rng.random_sample() * percent * N_MASK)
            mask[i, rng.choice(np.arange(N_MASK), replace=False, size=masked)] = 0
    return mask


def _get_transform(center, scale, rot):
    """imutils.py:12-36 at res = (256, 256)"""
    h = 200 * scale
    t = np.zeros((3, 3))
    t[0, 0] = t[1, 1] = float(RES) / h
    t[0, 2] = RES * (-float(center[0]) / h + .5)
    t[1, 2] = RES * (-float(center[1]) / h + .5)
    t[2, 2] = 1
    if not rot == 0:
        a = -rot * np.pi / 180
        sn, cs = np.sin(a), np.cos(a)
        turn = np.array([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1.0]])
        there, back = np.eye(3), np.eye(3)
        there[:2, 2] = -RES / 2
        back[:2, 2] = RES / 2
        t = np.dot(back, np.dot(turn, np.dot(there, t)))
    return t


def _apply(t, x, y):
    """(t . (x, y, 1))[:2] as (t0 x + t1 y) + t2: the summation order the label kernel uses"""
    return np.array([(t[0, 0] * x + t[0, 1] * y) + t[0, 2], (t[1, 0] * x + t[1, 1] * y) + t[1, 2]])


def crop_geometry(center, scale, rot):
    """imutils.py:56-66 -> (ul, br) of rot = 0 and pad, with the reference's truncations"""
    tinv = np.linalg.inv(_get_transform(center, scale, 0))
    ul = _apply(tinv, 0.0, 0.0).astype(int)                       # transform([1, 1], invert=1) - 1
    br = _apply(tinv, float(RES), float(RES)).astype(int)
    pad = int(np.linalg.norm(br - ul) / 2 - float(br[1] - ul[1]) / 2)
    return ul, br, pad


def _f64(a, shape):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    assert a.shape[1:] == shape, (a.shape, shape)
    return a


class TrainBatchMaker:
    """labels: dict of the dataset's annotation arrays -- ``center`` [N, 2], ``scale`` [N], and optionally ``pose`` [N, 72] + ``shape`` [N, 10]
    (+ ``has_smpl`` [N]), ``part`` [N, 24, 3], ``openpose`` [N, 25, 3], ``S`` [N, 24, 4], ``smpl_2dkps`` [N, 24, 3], ``gender`` [N] ('m' / other);
    missing ones default as base_dataset.py:74-130 does.  They are uploaded once (float64) and stay on ``device``."""

    def __init__(self, labels, device, rot_factor=30, noise_factor=0.4, scale_factor=0.25, is_train=True, ignore_3d=False):
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('TrainBatchMaker runs on a HIP device only (no CPU fallback)')
        self.device, self.is_train = device, is_train
        self.factors = dict(rot_factor=rot_factor, noise_factor=noise_factor, scale_factor=scale_factor)
        self.center = _f64(labels['center'], (2,))
        self.scale = np.asarray(labels['scale'], dtype=np.float64).reshape(-1)
        n = self.n = len(self.scale)
        up = lambda a: torch.from_numpy(a).to(device)
        if 'pose' in labels and 'shape' in labels:
            self.pose, self.betas = up(_f64(labels['pose'], (72,))), up(_f64(labels['shape'], (10,)))
            has_smpl = np.asarray(labels['has_smpl'], dtype=np.float32) if 'has_smpl' in labels else np.ones(n, dtype=np.float32)
        else:
            self.pose = self.betas = None
            has_smpl = np.zeros(n, dtype=np.float32)
        if ignore_3d:
            has_smpl = np.zeros(n, dtype=np.float32)
        self.has_smpl = up(np.ascontiguousarray(has_smpl))
        part = _f64(labels['part'], (24, 3)) if 'part' in labels else np.zeros((n, 24, 3))
        openpose = _f64(labels['openpose'], (25, 3)) if 'openpose' in labels else np.zeros((n, 25, 3))
        self.keypoints = up(np.ascontiguousarray(np.concatenate([openpose, part], axis=1)))
        self.S = up(_f64(labels['S'], (24, 4))) if 'S' in labels and not ignore_3d else None
        self.smpl_2dkps = up(_f64(labels['smpl_2dkps'], (24, 3))) if 'smpl_2dkps' in labels else None
        gender = np.array([0 if str(g) == 'm' else 1 for g in labels['gender']]) if 'gender' in labels else -np.ones(n)
        self.gender = up(np.ascontiguousarray(gender.astype(np.int32)))

    @torch.no_grad()
    def __call__(self, images, sample_index, params=None, kp_is_smpl=False, meta_mask=None, want_raw=False):
        """images: list of B uint8 [H_i, W_i, 3] RGB tensors on the device (numpy arrays are uploaded, once each; sizes may differ);
        sample_index: B indices into the annotation arrays; params: (flip, pn, rot, sc) as ``draw_augm_params`` returns them (None: drawn here,
        which also draws meta_mask unless given); kp_is_smpl: the 'surreal' joint convention of flip_kp.
        -> dict of device tensors with the keys and dtypes of ``__getitem__`` stacked over the batch; ``img`` is [B, 3, 256, 192] (columns 32 .. 223
        computed directly).  want_raw adds ``img_u8`` [B, 256, 192, 3], the patch before ``/ 255``."""
        dev = self.device
        imgs = []
        for im in images:
            if isinstance(im, np.ndarray):
                im = torch.from_numpy(np.ascontiguousarray(im)).to(dev)
            if not im.is_cuda:
                raise RuntimeError('TrainBatchMaker needs images on a HIP device (no CPU fallback)')
            assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.stride(2) == 1 and im.stride(1) == 3
            imgs.append(im)
        index = np.asarray(sample_index, dtype=np.int64).reshape(-1)
        B = len(index)
        assert len(imgs) == B and B > 0 and index.min() >= 0 and index.max() < self.n
        if params is None:
            params = draw_augm_params(B, is_train=self.is_train, **self.factors)
        if meta_mask is None:
            meta_mask = draw_meta_mask(B, is_train=self.is_train)
        flip, pn, rot, sc = (np.asarray(p) for p in params)
        meta_mask = np.ascontiguousarray(meta_mask, dtype=np.uint8).reshape(B, N_MASK)

        rows, rot_off, mid_off, coef_off, max_w, max_h = [], 0, 0, 0, 1, 1
        for b in range(B):
            i, r = index[b], float(rot[b])
            center, scale = self.center[i], float(sc[b]) * self.scale[i]
            ul, br, pad = crop_geometry(center, scale, r)
            bw, bh = int(br[0] - ul[0]), int(br[1] - ul[1])
            if bw < 1 or bh < 1 or (r != 0 and pad < 1):
                raise ValueError('sample %d: empty crop box (scale %g)' % (i, scale))
            if r == 0:
                pad, M = 0, np.zeros(6)
            else:
                th = np.deg2rad(r)
                cs, sn = np.cos(th), np.sin(th)
                cx, cy = (bw + 2 * pad) / 2 - 0.5, (bh + 2 * pad) / 2 - 0.5
                M = np.array([cs, -sn, cx - cs * cx + sn * cy, sn, cs, cy - sn * cx - cs * cy])
            kx, ky = (int(np.ceil(2.0 * max(float(s) / RES, 1.0))) * 2 + 1 for s in (bw, bh))
            a3, aa = -r * np.pi / 180, np.deg2rad(-r)
            im = imgs[b]
            rows.append(struct.pack(L.AUGMENT_ITEM_FORMAT, im.data_ptr(), im.stride(0), int(i), rot_off, mid_off, coef_off,
                                    im.shape[0], im.shape[1], int(ul[0]), int(ul[1]), bw, bh, pad, int(flip[b]), int(bool(kp_is_smpl)), kx, ky, 0,
                                    *_get_transform(center, scale, r).reshape(-1), *M, np.cos(a3), np.sin(a3), np.cos(aa), np.sin(aa),
                                    *(float(v) for v in pn[b]), r, scale, float(center[0]), float(center[1])))
            if pad:
                rot_off += bw * bh * 3
            mid_off += bh * (X_SLICE[1] - X_SLICE[0]) * 3
            coef_off += RES * (4 + kx + ky)
            max_w, max_h = max(max_w, bw), max(max_h, bh)
        item_bytes = struct.calcsize(L.AUGMENT_ITEM_FORMAT)
        table = torch.frombuffer(bytearray(b''.join(rows) + meta_mask.tobytes()), dtype=torch.uint8).to(dev)     # the one upload of the call
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=dev)
        rot_scratch = new(rot_off, dtype=torch.uint8) if rot_off else None
        mid_scratch, coef_scratch = new(mid_off, dtype=torch.uint8), new(coef_off, dtype=torch.int32)
        out = {'img': new(B, 3, RES, X_SLICE[1] - X_SLICE[0])}
        raw = new(B, RES, X_SLICE[1] - X_SLICE[0], 3, dtype=torch.uint8) if want_raw else None
        L.augment_crop(table, B, max_w, max_h, rot_off > 0, rot_scratch, mid_scratch, coef_scratch, out['img'], raw, MEAN, STD)
        if want_raw:
            out['img_u8'] = raw
        out.update(pose=new(B, 72), betas=new(B, 10), keypoints=new(B, 49, 3), keypoints_world=new(B, 49, 3), smpl_2dkps=new(B, 24, 3),
                   pose_3d=new(B, 24, 4), meta_mask=new(B, N_MASK, 1), has_smpl=new(B), has_pose_3d=new(B, dtype=torch.int64),
                   scale=new(B, dtype=torch.float64), center=new(B, 2), orig_shape=new(B, 2, dtype=torch.int64),
                   is_flipped=new(B, dtype=torch.int64), rot_angle=new(B), gender=new(B, dtype=torch.int32),
                   sample_index=new(B, dtype=torch.int64), bbox_height=new(B), bbox_width=new(B), focal=new(B), bbox_info=new(B, 5))
        io = L._WhmrAugmentLabelsIO()
        for k in ('pose', 'betas', 'keypoints', 'S', 'smpl_2dkps', 'has_smpl', 'gender'):
            setattr(io, k, L._ptr(getattr(self, k)))
        io.mask = table.data_ptr() + B * item_bytes
        for k, _ in L._WhmrAugmentLabelsIO._fields_:
            if k.startswith('o_'):
                setattr(io, k, out[k[2:]].data_ptr())
        L.augment_labels(table, B, io)
        return out
