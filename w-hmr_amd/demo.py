"""Per-frame inference pipeline on the device: the input preparation of demo/tester.py:95-146 + the model call of :150-162.

    out = infer_frame(model, frame_u8, dets)        # frame: uint8 [H, W, 3] RGB, dets: [(c_x, c_y, w, h), ...] person boxes

What the reference does per frame on the CPU -- one cv2.warpAffine + ToTensor + Normalize per detection, bbox_info in numpy,
PIL resize of the full image, then ``full_x`` replicated once per person -- happens here in a handful of launches: the frame is
uploaded once, ``crop_persons`` cuts and normalises all person patches in one launch (only the 192 columns the model reads), the
camera-calibration ResNet-50 sees the resized frame ONCE (batch-1 ``full_x`` is broadcast), and the meta tensors
are a few dozen floats computed on the host.

    out = infer_clip(model, frames, dets_per_frame)  # a clip: all persons of F frames in ONE model call (ClipPipeline: replayed from a HIP graph)

For a clip two launches prepare everything: ``crop_persons_frames`` (all patches of all frames) and ``full_image_input_pillow`` (the camera input of
all frames, Pillow's 8-bit bilinear resize bit for bit); the camera model runs at batch F and ``frame_index`` hands each person their frame's camera.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from .datasets.img_utils import MEAN, STD, _clip_frames, crop_persons, crop_persons_frames


def frame_meta(dets, orig_h, orig_w, device):
    """demo/tester.py:110-146: center, scale (= w / 200), bbox_height, orig_shape (H, W) and the CLIFF-style bbox_info."""
    d = np.asarray(dets, dtype=np.float64).reshape(-1, 4)
    n = d.shape[0]
    scale = d[:, 2] / 200.
    focal = math.sqrt(orig_h ** 2 + orig_w ** 2)                                       # pesudo_focal, tester.py:134-136
    cx, cy = d[:, 0] - orig_w / 2., d[:, 1] - orig_h / 2.
    info = np.stack([cx, cy, 200. * scale, np.full(n, float(orig_w)), np.full(n, float(orig_h))], 1) / np.float32(focal)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    return dict(center=t(d[:, :2]), scale=t(scale), bbox_height=t(200. * scale),
                orig_shape=t(np.tile(np.array([[orig_h, orig_w]], dtype=np.float32), (n, 1))), bbox_info=t(info.astype(np.float32)))


def resize_target(H, W, short_side=600):
    """(h, w) of torchvision's Resize(short_side) on an H x W image (tester.py:47-53): the short side becomes short_side, the aspect is kept"""
    return (short_side, int(short_side * W / H)) if H <= W else (int(short_side * H / W), short_side)


@torch.no_grad()
def full_image_input_pillow(frames_u8, short_side=600, want_u8=False):
    """tester.py:47-53,101-103 for F frames of one size in two launches: Resize(short side) EXACTLY as Pillow's 8-bit Image.resize(..., BILINEAR)
    computes it -> ToTensor -> Normalize.  frames_u8: uint8 [F, H, W, 3] (or one [H, W, 3] frame) on the HIP device, numpy is uploaded once.
    Returns fp32 [F, 3, h, w]; with want_u8 also the resized uint8 frames [F, h, w, 3]."""
    if isinstance(frames_u8, np.ndarray):
        frames_u8 = torch.from_numpy(np.ascontiguousarray(frames_u8)).cuda()
    if frames_u8.dim() == 3:
        frames_u8 = frames_u8.unsqueeze(0)
    if not frames_u8.is_cuda:
        raise RuntimeError('full_image_input_pillow runs on a HIP device only (no CPU fallback)')
    frames_u8 = frames_u8.contiguous()
    F_, H, W = frames_u8.shape[:3]
    h, w = resize_target(H, W, short_side)
    dev = frames_u8.device
    coef = L.resize_coeffs(H, W, h, w, dev)
    mid = torch.empty(F_ * H * L.resize_mid_pitch(w), dtype=torch.uint8, device=dev)                   # the horizontal pass's uint8 intermediate
    out = torch.empty(F_, 3, h, w, dtype=torch.float32, device=dev)
    out_u8 = torch.empty(F_, h, w, 3, dtype=torch.uint8, device=dev) if want_u8 else None
    L.resize_normalize_frames(frames_u8, h, w, coef, mid, out, out_u8, MEAN, STD)
    return (out, out_u8) if want_u8 else out


@torch.no_grad()
def full_image_input(frame_u8, short_side=600, full_image='torch'):
    """tester.py:47-53,101-103: Resize(short side 600, bilinear + antialias like PIL) -> ToTensor -> Normalize, [1, 3, h, w] fp32.
    full_image='pillow': the resize is Pillow's 8-bit resampler bit for bit (``full_image_input_pillow``, what the clip path uses); the default
    'torch' interpolates in float and is only close to it."""
    if full_image == 'pillow':
        return full_image_input_pillow(frame_u8, short_side)
    if full_image != 'torch':
        raise ValueError("full_image is 'torch' or 'pillow', got %r" % (full_image,))
    H, W = frame_u8.shape[:2]
    s = short_side / min(H, W)
    h, w = resize_target(H, W, short_side)
    x = frame_u8.permute(2, 0, 1).unsqueeze(0).float()
    if (h, w) != (H, W):
        x = F.interpolate(x, size=(h, w), mode='bilinear', align_corners=False, antialias=s < 1).round_().clamp_(0, 255)
    mean = torch.tensor(MEAN, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, device=x.device).view(1, 3, 1, 1)
    return (x / 255. - mean) / std


@torch.no_grad()
def prepare_frame(frame_u8, dets, with_full_image=True, full_image='torch'):
    """frame_u8: uint8 [H, W, 3] RGB on the HIP device (or numpy: uploaded once).  Returns the keyword arguments of WHMR.forward."""
    if isinstance(frame_u8, np.ndarray):
        frame_u8 = torch.from_numpy(np.ascontiguousarray(frame_u8)).cuda()
    H, W = frame_u8.shape[:2]
    kw = frame_meta(dets, H, W, frame_u8.device)
    kw['x'] = crop_persons(frame_u8, dets, crop_size=256, scale=1.0, x_slice=(32, 224))        # == inp_images[:, :, :, 32:-32]
    kw['full_x'] = full_image_input(frame_u8, full_image=full_image) if with_full_image else None
    return kw


@torch.no_grad()
def infer_frame(model, frame_u8, dets, with_full_image=True, full_image='torch'):
    """One frame, all detected persons: the vis_dict of WHMR.forward (tester.py:150-165)."""
    kw = prepare_frame(frame_u8, dets, with_full_image, full_image)
    return model(x=kw['x'], meta_masks=None, center=kw['center'], scale=kw['scale'], bbox_height=kw['bbox_height'],
                 orig_shape=kw['orig_shape'], bbox_info=kw['bbox_info'], is_train=False, J_regressor=None, full_x=kw['full_x'])


@torch.no_grad()
def render_frame(out, frame_u8, renderer, per_person=False):
    """The picture of a frame (tester.py:176-214, overlay panel): ``local_smpl_vertices`` of the vis_dict ``out`` drawn over ``frame_u8`` with
    ``pred_cam_t`` / ``focal_length``, identity camera rotation (tester.py:194) and the frame centre (:185) by ``renderer``
    (utils.renderer_cam.MeshRenderer).  uint8 [H, W, 3] with all persons in one depth buffer, or [P, H, W, 3] with per_person.  No host sync."""
    if isinstance(frame_u8, np.ndarray):
        frame_u8 = torch.from_numpy(np.ascontiguousarray(frame_u8)).cuda()
    return renderer.render(frame_u8, out['local_smpl_vertices'], out['pred_cam_t'], out['focal_length'], per_person=per_person)


class FramePipeline:
    """infer_frame with the model call (cam_model + W-HMR forward, ~200 launches) replayed from a HIP graph per (number of persons,
    full-image size): at one to a few persons per frame the eager path is bound by Python launch overhead, not by the GPU.
    With ``renderer`` (utils.renderer_cam.MeshRenderer) the call returns (vis_dict, image): the overlay is launched right behind the replayed graph on
    the same stream, with no host sync between model and picture."""

    def __init__(self, model, with_full_image=True, renderer=None, per_person=False, full_image='torch'):
        self.model, self.with_full_image, self._graphs = model, with_full_image, {}
        self.renderer, self.per_person, self.full_image = renderer, per_person, full_image

    @torch.no_grad()
    def __call__(self, frame_u8, dets):
        from .graph import GraphedForward
        if self.renderer is not None and isinstance(frame_u8, np.ndarray):
            frame_u8 = torch.from_numpy(np.ascontiguousarray(frame_u8)).cuda()             # uploaded once for crops and picture
        kw = prepare_frame(frame_u8, dets, self.with_full_image, self.full_image)
        key = (kw['x'].shape[0], tuple(kw['full_x'].shape) if kw['full_x'] is not None else None)
        call = dict(x=kw['x'], meta_masks=None, center=kw['center'], scale=kw['scale'], bbox_height=kw['bbox_height'],
                    orig_shape=kw['orig_shape'], bbox_info=kw['bbox_info'], is_train=False, J_regressor=None, full_x=kw['full_x'])
        g = self._graphs.get(key)
        if g is None:
            g = self._graphs[key] = GraphedForward(self.model, **call)
        out = g(**call)
        if self.renderer is None:
            return out
        return out, render_frame(out, frame_u8, self.renderer, self.per_person)


# ----------------------------------------------------------------------------- clip inference: all persons of many frames in one model call
def padded_count(P, pad_to=None):
    """the person batch of a clip with P detections: P, or the next multiple of pad_to (rows P .. repeat the last detection)"""
    if pad_to is None:
        return P
    if pad_to < 1:
        raise ValueError('pad_to must be a positive integer, got %r' % (pad_to,))
    return -(-P // pad_to) * pad_to


def _frame_shapes(frames):
    if torch.is_tensor(frames) or isinstance(frames, np.ndarray):
        if frames.ndim != 4:
            raise ValueError('one tensor of frames is [F, H, W, 3], got %s' % (tuple(frames.shape),))
        return [tuple(frames.shape[1:3])] * frames.shape[0]
    return [tuple(f.shape[:2]) for f in frames]


def clip_plan(frames, dets_per_frame, with_full_image=True, pad_to=None):
    """Host-side layout of a clip, decided before anything touches the device: (P, padded P, per-frame (H, W), the flat list of padded P detections,
    their frame indices as int64 numpy).  Returns None for a clip without any detection; raises ValueError when with_full_image meets frames of
    different sizes (the camera model sees the clip as one [F, 3, h, w] batch)."""
    shapes = _frame_shapes(frames)
    if len(shapes) != len(dets_per_frame):
        raise ValueError('%d frames but detections for %d' % (len(shapes), len(dets_per_frame)))
    if with_full_image and len(set(shapes)) > 1:
        raise ValueError('with_full_image needs all frames of a clip to have one size (got %s); pass with_full_image=False or split the clip'
                         % sorted(set(shapes)))
    dets = [tuple(float(v) for v in d) for ds in dets_per_frame for d in ds]
    P = len(dets)
    if P == 0:
        return None
    index = np.repeat(np.arange(len(shapes), dtype=np.int64), [len(d) for d in dets_per_frame])
    Pp = padded_count(P, pad_to)
    dets = dets + [dets[-1]] * (Pp - P)
    index = np.concatenate([index, np.full(Pp - P, index[-1], dtype=np.int64)])
    return P, Pp, shapes, dets, index


def clip_meta(dets, index, shapes, device):
    """``frame_meta`` for the persons of a clip: every row uses the size of ITS frame (same arithmetic per row)"""
    parts = [frame_meta([d], shapes[f][0], shapes[f][1], 'cpu') for d, f in zip(dets, index)]
    return {k: torch.cat([p[k] for p in parts]).pin_memory().to(device, non_blocking=True) for k in parts[0]}


@torch.no_grad()
def prepare_clip(frames, dets_per_frame, with_full_image=True, pad_to=None, want_frames=False):
    """-> (keyword arguments of WHMR.forward for the whole clip, P) or None (no detection).  Two input launches for the whole clip: all person crops
    (``crop_persons_frames``) and, with_full_image, the Pillow-exact camera input of all F frames (``full_image_input_pillow``)."""
    plan = clip_plan(frames, dets_per_frame, with_full_image, pad_to)
    if plan is None:
        return None
    P, Pp, shapes, dets, index = plan
    if with_full_image and not torch.is_tensor(frames) and not isinstance(frames, np.ndarray):
        frames = np.stack(frames) if isinstance(frames[0], np.ndarray) else torch.stack(list(frames))     # one [F, H, W, 3] block
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()                                    # one upload for crops and camera input
    frame_list = _clip_frames(frames)
    per_frame = [[] for _ in shapes]
    for d, f in zip(dets, index):
        per_frame[f].append(d)                                                 # the padding rows repeat the last detection, in its frame: still frame order
    x, index_d = crop_persons_frames(frame_list, per_frame, crop_size=256, scale=1.0, x_slice=(32, 224))
    kw = clip_meta(dets, index, shapes, x.device)
    kw['x'] = x
    kw['full_x'] = full_image_input_pillow(frames) if with_full_image else None
    kw['frame_index'] = index_d
    if want_frames:
        kw['frames'] = frame_list
    return kw, P


def _clip_call(kw):
    return dict(x=kw['x'], meta_masks=None, center=kw['center'], scale=kw['scale'], bbox_height=kw['bbox_height'], orig_shape=kw['orig_shape'],
                bbox_info=kw['bbox_info'], is_train=False, J_regressor=None, full_x=kw['full_x'],
                frame_index=kw['frame_index'] if kw['full_x'] is not None else None)


def _clip_result(out, kw, P):
    out = {k: v[:P] for k, v in out.items()}                                   # the padding rows leave here
    out['frame_index'] = kw['frame_index'][:P]
    return out


@torch.no_grad()
def infer_clip(model, frames, dets_per_frame, with_full_image=True, pad_to=None):
    """All persons of all frames of a clip in ONE model call.  frames: list of uint8 [H_i, W_i, 3] RGB frames (device tensors or numpy) or one
    [F, H, W, 3] tensor; dets_per_frame: per frame its [(c_x, c_y, w, h), ...], possibly empty.  Returns the vis_dict of WHMR.forward with one row per
    person (frame order, then detection order) plus ``frame_index`` int64 [P]; None for a clip without any detection.  With with_full_image the
    camera model runs once per FRAME (batch F, Pillow-exact input) and all frames must have one size (ValueError otherwise).  pad_to=k pads the
    person batch to the next multiple of k by repeating the last detection; every output is sliced back to P rows."""
    prep = prepare_clip(frames, dets_per_frame, with_full_image, pad_to)
    if prep is None:
        return None
    kw, P = prep
    return _clip_result(model(**_clip_call(kw)), kw, P)


class ClipPipeline:
    """infer_clip with the model call replayed from a HIP graph per (padded person count, number of frames, frame size); the input preparation
    (two launches per clip) stays outside the graph, as in FramePipeline.  person_bucket: the person batch is padded to its next multiple, so clips of
    similar size share a graph.  With ``renderer`` (utils.renderer_cam.MeshRenderer) the call returns (vis_dict, [F overlay images]): one
    ``render_frame`` launch group per frame over that frame's rows, behind the replayed graph on the same stream, no host sync; a frame without
    detections comes back as a copy of itself."""

    def __init__(self, model, with_full_image=True, person_bucket=8, renderer=None):
        self.model, self.with_full_image, self.person_bucket, self.renderer, self._graphs = model, with_full_image, person_bucket, renderer, {}

    @torch.no_grad()
    def __call__(self, frames, dets_per_frame):
        from .graph import GraphedForward
        prep = prepare_clip(frames, dets_per_frame, self.with_full_image, self.person_bucket, want_frames=self.renderer is not None)
        if prep is None:
            return None
        kw, P = prep
        call = _clip_call(kw)
        key = (kw['x'].shape[0], len(dets_per_frame), tuple(kw['full_x'].shape[2:]) if kw['full_x'] is not None else None)
        g = self._graphs.get(key)
        if g is None:
            g = self._graphs[key] = GraphedForward(self.model, **call)
        out = _clip_result(g(**call), kw, P)
        if self.renderer is None:
            return out
        images, row = [], 0
        for frame, dets in zip(kw['frames'], dets_per_frame):
            n = len(dets)
            images.append(render_frame({k: out[k][row:row + n] for k in ('local_smpl_vertices', 'pred_cam_t', 'focal_length')}, frame, self.renderer)
                          if n else frame.clone())
            row += n
        return out, images
