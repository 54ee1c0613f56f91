"""Training batches on the device: the sample-making of ``BaseDataset.__getitem__`` (datasets/base_dataset.py:249-384) for a whole batch behind
one call, producing the dictionary ``core/trainer.py:383-403`` reads.

The reference makes every sample on the CPU: it draws the augmentation (``augm_params``), cuts / rotates the person box (utils/imutils.py:crop),
resizes it with Pillow, flips it, scales the colour channels, normalises, and pushes keypoints, 3-D joints and the SMPL pose through the same flip /
rotation / scale.  Here the annotation arrays are uploaded once (``TrainBatchMaker``), and per batch the host computes -- in float64 numpy, exactly as
the reference does -- only the per-sample geometry (box corners and pad with their ``int`` truncations, the 3 x 3 ``get_transform`` matrix, the
rotation's inverse map, the occluders' rectangles) and uploads it as ONE table (struct whmr_augment_item, include/whmr_hip.h) that also names every source image by pointer,
size and row stride.  Everything per pixel and per label runs in csrc/augment.hip (five launches, no host synchronisation).

Stages of the image: 1. integer box, 2. rotation, 3. Pillow's bicubic resize, 4. flip, 4a. occluders, 5. colour noise + normalise (csrc/augment.hip).

4a. occluders (``USE_SYNTHETIC_OCCLUSION``, on by default in the reference: base_dataset.py:192-194 pastes Pascal VOC objects onto every training
sample with PARE's ``occlude_with_pascal_objects``): give ``TrainBatchMaker`` the list of RGBA objects PARE's ``load_pascal_occluders`` (or its
cached pickle) yields.  They are packed once into a resident ``OccluderBank``; per batch ``draw_occlusions`` draws, per sample, 1 .. 7 pastes of
(object, factor in [0.2, 1], centre in the 256 x 256 patch), the host turns each into an integer rectangle in float64 as numpy does (sizes
``np.round((w, h) * factor)``, ``start = np.round(centre) - size // 2``) and the rows travel in the call's one upload.  The device resizes the
object by AREA AVERAGING and alpha-blends it (``a = fp32(A) / 255; dst = uint8(a src + (1 - a) dst)``) inside the vertical-pass launch.  The
resize is defined here in integers so that host and device agree to the bit: along an axis of source length S resized to n, output u covers
[u S, (u + 1) S) and source texel j covers [j n, (j + 1) n) in units of 1 / n texel; the weight is the integer overlap (the weights of an axis sum
to S); a resized channel, alpha included, is ``(2 sum(wy wx v) + D) // (2 D)`` with D = w h (round half up).  That is within 0.5 of the float64
area average (at most one grey level from cv2's INTER_AREA at ties), the identity at n == S and the rounded block mean at integer ratios.  PARE and
cv2 are not available where this was written: parity with PARE / cv2 is unpinned (as skimage's rotation is).

Out of scope (the image differs from the reference's where these are switched on): the albumentations ``ColorJitter`` (p = 0.2; its arithmetic and
random order are not pinned here), ``agora_crop``'s special case (no crop) and reading the occluders out of a Pascal VOC tree (cv2 morphology).
A sample whose crop raises in the reference (base_dataset.py:282-287 then retries with the unscaled box) raises here.
Image decoding stays with the caller.
"""
import random
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


def draw_occlusions(n, n_occluders, rng=np.random, pyrng=random):
    """the draws of ``occlude_with_pascal_objects`` for n samples -> list of n float64 arrays [k_i, 4] = (occluder index, factor, cx, cy).  Per sample
    ``count = rng.randint(1, 8)``, then per paste ``random.choice(occluders)`` (Python's generator: ``pyrng.randrange`` consumes the same stream),
    ``rng.uniform(0.2, 1.0)`` and ``rng.uniform([0, 0], [256, 256])``, in this order: the same seeds give the same numbers."""
    out = []
    for _ in range(n):
        rows = np.zeros((rng.randint(1, 8), 4))
        for row in rows:
            row[0] = pyrng.randrange(n_occluders)
            row[1] = rng.uniform(0.2, 1.0)
            row[2:] = rng.uniform([0, 0], [RES, RES])
        out.append(rows)
    return out


def plan_occlusions(occlusions, sizes):
    """occlusions: per sample [k, 4] (occluder index, factor, cx, cy) as ``draw_occlusions`` returns them; sizes: int [n_occluders, 2] = (h, w).
    -> (pastes int32 [n_pastes, 5] = (index, nw, nh, start_x, start_y), row pointers int32 [B + 1]), in float64 / int arithmetic as the reference
    runs it: ``(nw, nh) = np.round((w, h) * factor).astype(int)`` (half to even), ``start = np.round(centre).astype(int32) - (nw, nh) // 2``.
    Dropped: a paste with nw == 0 or nh == 0 (the reference raises inside cv2 and retries the whole sample), and one whose rectangle misses the
    kept columns 32 .. 223 or the rows 0 .. 255.  An index outside the bank raises ValueError."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    occ = [np.asarray(o, dtype=np.float64).reshape(-1, 4) for o in occlusions]
    allp = np.concatenate(occ + [np.zeros((0, 4))])                # one vectorised pass over the pastes of the batch
    k, factor = allp[:, 0], allp[:, 1]
    if not np.isfinite(allp).all():
        raise ValueError('occlusions hold a non-finite number')
    if not ((k == np.floor(k)) & (k >= 0) & (k < len(sizes))).all():
        raise ValueError('occluder index outside the bank of %d: %r' % (len(sizes), k[~((k == np.floor(k)) & (k >= 0) & (k < len(sizes)))][:4]))
    if not ((factor >= 0.0) & (factor <= 1.0)).all():
        raise ValueError('occluder factor outside [0, 1] (the resize only shrinks)')
    k = k.astype(np.int64)
    n = np.round(sizes[k][:, ::-1] * factor[:, None]).astype(int)                         # (nw, nh)
    start = np.round(allp[:, 2:]).astype(np.int32) - n // 2
    keep = ((n > 0).all(1) & (start[:, 0] + n[:, 0] > X_SLICE[0]) & (start[:, 0] < X_SLICE[1]) & (start[:, 1] + n[:, 1] > 0) & (start[:, 1] < RES))
    sample = np.repeat(np.arange(len(occ)), [len(o) for o in occ])
    ptr = np.concatenate([[0], np.cumsum(np.bincount(sample[keep], minlength=len(occ)))])
    rows = np.concatenate([k[:, None], n, start], axis=1)[keep]
    return np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 5), ptr.astype(np.int32)


class OccluderBank:
    """occluders: list of uint8 [h, w, 4] RGBA arrays (what PARE's ``load_pascal_occluders`` yields), packed once into one byte buffer on ``device``
    (``bank``) plus an int64 table [n, 3] of (byte offset, h, w) per object (``table``); ``sizes`` [n, 2] = (h, w) stays on the host for the
    per-batch plan.  ValueError: an empty list, anything that is not uint8 [h, w, 4] with h, w >= 1, a side above 32767 or 255 h w >= 2^31 (the
    device sums a resized texel in 32 bits)."""

    def __init__(self, occluders, device):
        occluders = list(occluders)
        if not occluders:
            raise ValueError('OccluderBank needs at least one occluder')
        table, off = [], 0
        for i, o in enumerate(occluders):
            if not (isinstance(o, np.ndarray) and o.dtype == np.uint8 and o.ndim == 3 and o.shape[2] == 4 and o.shape[0] >= 1 and o.shape[1] >= 1):
                raise ValueError('occluder %d is not a uint8 [h, w, 4] RGBA array with h, w >= 1' % i)
            h, w = o.shape[:2]
            if max(h, w) > 32767 or 255 * h * w >= 2 ** 31:
                raise ValueError('occluder %d (%d x %d) is too large for the 32-bit area sum' % (i, h, w))
            table.append((off, h, w))
            off += h * w * 4
        self.device = torch.device(device)
        self.sizes = np.array([t[1:] for t in table], dtype=np.int64)
        self.bank = torch.from_numpy(np.concatenate([np.ascontiguousarray(o).reshape(-1) for o in occluders])).to(self.device)
        self.table = torch.tensor(table, dtype=torch.int64).to(self.device)

    def __len__(self):
        return len(self.sizes)


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
    missing ones default as base_dataset.py:74-130 does.  They are uploaded once (float64) and stay on ``device``.  occluders: None, a list of uint8
    [h, w, 4] RGBA objects or an ``OccluderBank`` on ``device``: switches stage 4a (synthetic occlusion) on for training batches."""

    def __init__(self, labels, device, rot_factor=30, noise_factor=0.4, scale_factor=0.25, is_train=True, ignore_3d=False, occluders=None):
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('TrainBatchMaker runs on a HIP device only (no CPU fallback)')
        self.device, self.is_train = device, is_train
        self.bank = None
        if occluders is not None:
            self.bank = occluders if isinstance(occluders, OccluderBank) else OccluderBank(occluders, device)
            if self.bank.bank.device != torch.empty(0, device=device).device:
                raise ValueError('the OccluderBank lives on %s, the maker on %s' % (self.bank.bank.device, device))
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

    def _occlusion_plan(self, occlusions, B):
        """the paste rows and row pointers of one call (``plan_occlusions``); occlusions None: drawn when the maker has a bank and is_train"""
        if occlusions is None:
            if self.bank is None or not self.is_train:
                return np.zeros((0, 5), dtype=np.int32), np.zeros(B + 1, dtype=np.int32)
            occlusions = draw_occlusions(B, len(self.bank))
        elif self.bank is None:
            raise ValueError('occlusions= given to a TrainBatchMaker without occluders')
        if len(occlusions) != B:
            raise ValueError('occlusions has %d entries for a batch of %d' % (len(occlusions), B))
        return plan_occlusions(occlusions, self.bank.sizes)

    @torch.no_grad()
    def __call__(self, images, sample_index, params=None, kp_is_smpl=False, meta_mask=None, want_raw=False, occlusions=None):
        """images: list of B uint8 [H_i, W_i, 3] RGB tensors on the device (numpy arrays are uploaded, once each; sizes may differ);
        sample_index: B indices into the annotation arrays; params: (flip, pn, rot, sc) as ``draw_augm_params`` returns them (None: drawn here,
        which also draws meta_mask unless given); kp_is_smpl: the 'surreal' joint convention of flip_kp.
        -> dict of device tensors with the keys and dtypes of ``__getitem__`` stacked over the batch; ``img`` is [B, 3, 256, 192] (columns 32 .. 223
        computed directly).  want_raw adds ``img_u8`` [B, 256, 192, 3], the patch before ``/ 255`` (occluded, after pn).
        occlusions: list of B arrays [k, 4] = (occluder index, factor, cx, cy) as ``draw_occlusions`` returns them, always applied (ValueError
        without a bank); None: drawn when the maker has occluders and is_train, between the draws of params and of meta_mask."""
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
        pastes, paste_ptr = self._occlusion_plan(occlusions, B)
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
        head = b''.join(rows) + meta_mask.tobytes()
        if len(pastes):                                            # the int32 paste rows and row pointers ride behind the mask, 4-byte aligned
            head += b'\0' * (-len(head) % 4)
            pastes_off, ptr_off = len(head), len(head) + pastes.nbytes
            head += pastes.tobytes() + paste_ptr.tobytes()
        table = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(dev)     # the one upload of the call
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=dev)
        rot_scratch = new(rot_off, dtype=torch.uint8) if rot_off else None
        mid_scratch, coef_scratch = new(mid_off, dtype=torch.uint8), new(coef_off, dtype=torch.int32)
        out = {'img': new(B, 3, RES, X_SLICE[1] - X_SLICE[0])}
        raw = new(B, RES, X_SLICE[1] - X_SLICE[0], 3, dtype=torch.uint8) if want_raw else None
        if len(pastes):
            L.augment_crop_occluded(table, B, max_w, max_h, rot_off > 0, rot_scratch, mid_scratch, coef_scratch, out['img'], raw, MEAN, STD,
                                    self.bank.bank, self.bank.table, table.data_ptr() + pastes_off, table.data_ptr() + ptr_off, len(pastes))
        else:
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
