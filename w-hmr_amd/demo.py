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

    sm = TrackSmoother(model);  out = infer_clip(model, frames, dets_per_frame, track_ids=ids_per_frame, smoother=sm)

With a ``renderer`` ClipPipeline also returns the clip's overlays, drawn by ONE launch group (``render_clip``: whmr_mesh_render_draws).

With a tracker's ids the rows of one person are linked over the frames (and over successive clips) and smoothed by a one-euro filter on the device
(``whmr_track_smooth``: one launch), and the vertices are recomputed from the smoothed pose and shape: what --smooth of demo/whmr_demo.py:135-144 asks for.
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


def _smpl_of(model):
    return model.regressor[0].smpl


@torch.no_grad()
def keypoints_full_image(model, out, sizes, frame_index=None):
    """The [P, 49, 3] keypoints (x, y, 1) of the vis_dict ``out`` in full-image pixels, which WHMR.forward does not return at inference: the 49
    joints of ``local_smpl_vertices`` (``SMPL.joints_from_vertices`` of the model's SMPL, so smoothed rows give smoothed keypoints) through the camera
    the overlay is drawn with -- ``pred_cam_t``, ``focal_length``, identity rotation, the frame centre (W // 2, H // 2) (tester.py:185,194).  sizes:
    (H, W) of the frame, or with frame_index (HOST integers, the frame of every row) one (H, W) per frame.  The third column is the confidence the
    ``keypoints_2d`` arguments of the renderer read: a prediction has none, so 1."""
    verts = out['local_smpl_vertices']
    P = verts.shape[0]
    if frame_index is None:
        per_row = [(int(sizes[0]), int(sizes[1]))] * P
    else:
        index = [int(i) for i in np.asarray(frame_index.cpu() if torch.is_tensor(frame_index) else frame_index).reshape(-1)]
        if len(index) != P:
            raise ValueError('%d rows but %d frame indices' % (P, len(index)))
        per_row = [(int(sizes[i][0]), int(sizes[i][1])) for i in index]
    joints = _smpl_of(model).joints_from_vertices(verts)
    center = torch.tensor([[w // 2, h // 2] for h, w in per_row], dtype=torch.float32).to(verts.device)
    xy = L.perspective(joints, None, out['pred_cam_t'].float().reshape(P, 3), out['focal_length'].float().reshape(P), center)
    return torch.cat([xy, torch.ones_like(xy[..., :1])], dim=2)


def _marks(model, out, wireframe, draw_keypoints):
    """the renderer's arguments for --wireframe / --draw_keypoints: the skeleton is that of the rows drawn, projected by the renderer itself"""
    kw = {}
    if wireframe:
        kw['wireframe'] = True
    if draw_keypoints:
        if model is None:
            raise ValueError('draw_keypoints needs the model: the joints come from its SMPL')
        kw['joints'] = _smpl_of(model).joints_from_vertices(out['local_smpl_vertices'])
    return kw


@torch.no_grad()
def render_frame(out, frame_u8, renderer, per_person=False, ground=False, wireframe=False, draw_keypoints=False, model=None, want=()):
    """The picture of a frame (tester.py:176-214, overlay panel): ``local_smpl_vertices`` of the vis_dict ``out`` drawn over ``frame_u8`` with
    ``pred_cam_t`` / ``focal_length``, identity camera rotation (tester.py:194) and the frame centre (:185) by ``renderer``
    (utils.renderer_cam.MeshRenderer).  uint8 [H, W, 3] with all persons in one depth buffer, or [P, H, W, 3] with per_person.  ground: True (or a
    height) puts the checkerboard ground plane under every person; a plane has one person's camera, so it needs per_person or a single person
    (ValueError otherwise).  wireframe: the meshes as hidden-line wireframe (--wireframe, whmr_demo.py:152); draw_keypoints: every person's
    keypoint skeleton under the mesh (--draw_keypoints, :158) -- the 49 joints of the rows drawn, from ``model``'s SMPL, so smoothed rows draw
    smoothed skeletons.  want: as MeshRenderer.render (a dict comes back; 'keypoints' = the projected joints).  No host sync."""
    if isinstance(frame_u8, np.ndarray):
        frame_u8 = torch.from_numpy(np.ascontiguousarray(frame_u8)).cuda()
    return renderer.render(frame_u8, out['local_smpl_vertices'], out['pred_cam_t'], out['focal_length'], per_person=per_person, ground=ground, want=want,
                           **_marks(model, out, wireframe, draw_keypoints))


@torch.no_grad()
def render_clip(out, frames, renderer, frame_index, per_person=False, ground=False, wireframe=False, draw_keypoints=False, model=None, want=()):
    """``render_frame`` for a whole clip in one launch group (MeshRenderer.render_clip): the rows of the vis_dict ``out`` drawn over their frames.
    frames: [F, H, W, 3] or a list of frames (device tensors; numpy is uploaded); frame_index: the frame of every row as HOST integers.  Returns a
    list of F uint8 images, each equal to ``render_frame`` on that frame's rows (a frame without rows: its own bytes), or P images with per_person.
    ground, wireframe, draw_keypoints (with ``model``) and want as for ``render_frame``, in the same launch group."""
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    elif not torch.is_tensor(frames):
        frames = [torch.from_numpy(np.ascontiguousarray(f)).cuda() if isinstance(f, np.ndarray) else f for f in frames]
    return renderer.render_clip(frames, out['local_smpl_vertices'], out['pred_cam_t'], out['focal_length'], frame_index, per_person=per_person, ground=ground,
                                want=want, **_marks(model, out, wireframe, draw_keypoints))


class FramePipeline:
    """infer_frame with the model call (cam_model + W-HMR forward, ~200 launches) replayed from a HIP graph per (number of persons,
    full-image size): at one to a few persons per frame the eager path is bound by Python launch overhead, not by the GPU.
    With ``renderer`` (utils.renderer_cam.MeshRenderer) the call returns (vis_dict, image): the overlay is launched right behind the replayed graph on
    the same stream, with no host sync between model and picture; ``ground``, ``wireframe``, ``draw_keypoints`` and ``want`` are handed to
    ``render_frame`` (with ``want`` the second value is the renderer's dict: 'image', 'keypoints', ...)."""

    def __init__(self, model, with_full_image=True, renderer=None, per_person=False, full_image='torch', ground=False, wireframe=False,
                 draw_keypoints=False, want=()):
        self.model, self.with_full_image, self._graphs = model, with_full_image, {}
        self.renderer, self.per_person, self.full_image, self.ground = renderer, per_person, full_image, ground
        self.wireframe, self.draw_keypoints, self.want = wireframe, draw_keypoints, tuple(want)

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
        return out, render_frame(out, frame_u8, self.renderer, self.per_person, self.ground, self.wireframe, self.draw_keypoints, self.model, self.want)


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
def infer_clip(model, frames, dets_per_frame, with_full_image=True, pad_to=None, track_ids=None, smoother=None):
    """All persons of all frames of a clip in ONE model call.  frames: list of uint8 [H_i, W_i, 3] RGB frames (device tensors or numpy) or one
    [F, H, W, 3] tensor; dets_per_frame: per frame its [(c_x, c_y, w, h), ...], possibly empty.  Returns the vis_dict of WHMR.forward with one row per
    person (frame order, then detection order) plus ``frame_index`` int64 [P]; None for a clip without any detection.  With with_full_image the
    camera model runs once per FRAME (batch F, Pillow-exact input) and all frames must have one size (ValueError otherwise).  pad_to=k pads the
    person batch to the next multiple of k by repeating the last detection; every output is sliced back to P rows.
    smoother (a TrackSmoother) with track_ids (per frame one id per detection, None = untracked): the rows of each id are smoothed over time, across
    successive calls too; the host table is decided (and its ValueErrors raised) before anything is launched."""
    plan = _smoothing_plan(smoother, track_ids, dets_per_frame)
    prep = prepare_clip(frames, dets_per_frame, with_full_image, pad_to)
    if prep is None:
        return None
    kw, P = prep
    out = _clip_result(model(**_clip_call(kw)), kw, P)
    return out if plan is None else smoother.run(out, plan)


class ClipPipeline:
    """infer_clip with the model call replayed from a HIP graph per (padded person count, number of frames, frame size); the input preparation
    (two launches per clip) stays outside the graph, as in FramePipeline.  person_bucket: the person batch is padded to its next multiple, so clips of
    similar size share a graph.  With ``renderer`` (utils.renderer_cam.MeshRenderer) the call returns (vis_dict, [F overlay images]): ONE
    ``render_clip`` launch group for the whole clip, each image what ``render_frame`` draws over that frame's rows, behind the replayed graph on the
    same stream, no host sync; a frame without detections comes back as a copy of itself; per_person: [P images], one person each.  With
    ``smoother`` (a TrackSmoother) and per-call ``track_ids`` the smoothing stage (one filter launch + two SMPL calls) runs behind the replayed graph on the same stream, outside the graph -- its table changes per clip, like the input preparation --
    and the renderer draws the smoothed rows; the padding rows never enter a track.  ``ground``, ``wireframe``, ``draw_keypoints`` and ``want`` are handed
    to ``render_clip``: the skeletons are those of the rows drawn, smoothed ones included."""

    def __init__(self, model, with_full_image=True, person_bucket=8, renderer=None, smoother=None, per_person=False, ground=False, wireframe=False,
                 draw_keypoints=False, want=()):
        self.model, self.with_full_image, self.person_bucket, self.renderer, self._graphs = model, with_full_image, person_bucket, renderer, {}
        self.smoother, self.per_person, self.ground = smoother, per_person, ground
        self.wireframe, self.draw_keypoints, self.want = wireframe, draw_keypoints, tuple(want)

    @torch.no_grad()
    def __call__(self, frames, dets_per_frame, track_ids=None):
        from .graph import GraphedForward
        plan = _smoothing_plan(self.smoother, track_ids, dets_per_frame)
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
        if plan is not None:
            out = self.smoother.run(out, plan)
        if self.renderer is None:
            return out
        index = np.repeat(np.arange(len(dets_per_frame)), [len(d) for d in dets_per_frame])       # from the detections: the host has them
        return out, render_clip(out, kw['frames'], self.renderer, index, self.per_person, self.ground, self.wireframe, self.draw_keypoints, self.model,
                                self.want)


# ----------------------------------------------------------------------------- temporal smoothing of tracked persons
def _smoothing_plan(smoother, track_ids, dets_per_frame):
    """the host half of the smoothing stage of a clip call, before anything is launched: None without smoother / track_ids"""
    if track_ids is None:
        return None
    if smoother is None:
        raise ValueError('track_ids need a smoother (TrackSmoother)')
    return smoother.plan_clip(dets_per_frame, track_ids)


class SmoothPlan:
    """What one smoothing call will do, decided on the host: the int32 table of whmr_track_smooth as numpy arrays (``offsets`` [T + 1], ``rows`` [P],
    ``gap`` [n_tracked], ``slot`` [T]; ``ids``: the T track ids in table order) and the host state the call leaves behind (``commit``)."""

    def __init__(self, offsets, rows, gap, slot, ids, commit):
        self.offsets, self.rows, self.gap, self.slot, self.ids, self.commit = offsets, rows, gap, slot, ids, commit
        self.P, self.T, self.n_tracked = len(rows), len(slot), len(gap)

    def table(self):
        return np.concatenate([self.offsets, self.rows, self.gap, self.slot]).astype(np.int32)


class TrackSmoother:
    """One-euro smoothing of tracked persons over the frames of a clip and across clips (--smooth / --min_cutoff / --beta of demo/whmr_demo.py:135-144;
    the reference parses the flags and never filters).  Time is counted in frames.  Per track the 24 local joint rotations and the global root
    rotation are filtered on SO(3), ``pred_cam_t``, ``focal_length`` and ``shape`` as scalars (``whmr_track_smooth``, csrc/smooth.hip: one launch);
    ``local_smpl_vertices`` / ``smpl_vertices`` are recomputed by the model's own SMPL from the smoothed shape and rotations; ``cam_rotmat`` and
    ``render_rotmat`` are per-frame camera outputs and pass through.

    The host never reads device memory: it keeps track id -> state slot and each track's last absolute frame number, and a running frame counter
    that advances by F per clip call.  A track unseen for more than ``max_gap`` frames restarts; ``reset(track_id)`` frees a slot.  ValueError, before
    anything is launched: one id twice in one frame, more live tracks than ``max_tracks``.  ``model`` may be None for host-side planning only."""

    def __init__(self, model, min_cutoff=0.004, beta=1.0, d_cutoff=1.0, max_tracks=64, max_gap=30):
        if not (0 < min_cutoff <= 1e30 and 0 <= beta <= 1e30 and 0 < d_cutoff <= 1e30):
            raise ValueError('min_cutoff and d_cutoff are positive, beta is not negative (got %r, %r, %r)' % (min_cutoff, beta, d_cutoff))
        if max_tracks < 1 or max_gap < 1:
            raise ValueError('max_tracks and max_gap are at least 1 (got %r, %r)' % (max_tracks, max_gap))
        self.model, self.min_cutoff, self.beta, self.d_cutoff = model, float(min_cutoff), float(beta), float(d_cutoff)
        self.max_tracks, self.max_gap = int(max_tracks), int(max_gap)
        self.frame_counter = 0                      # absolute number of the next clip's first frame
        self._slots, self._last = {}, {}            # track id -> state slot, track id -> absolute frame number of its last sample
        self._state = None                          # device arrays, allocated with the first launch
        self.rotmats = None                         # (local_rotmat, global_rotmat) [P, 24, 3, 3] of the last call

    def reset(self, track_id=None):
        """forget one track (its slot is free again; the id starts a new track when it returns) or, without an id, all tracks and the frame counter"""
        if track_id is None:
            self._slots, self._last, self.frame_counter = {}, {}, 0
        else:
            self._slots.pop(track_id, None)
            self._last.pop(track_id, None)

    # ---- host
    def plan(self, track_ids, frame_numbers):
        """-> SmoothPlan for rows with these ids (None: untracked) at these absolute frame numbers.  Changes nothing: ``run`` commits the plan."""
        ids, frames = list(track_ids), [int(f) for f in frame_numbers]
        if len(ids) != len(frames):
            raise ValueError('%d track ids but %d frame numbers' % (len(ids), len(frames)))
        tracks = {}                                                               # id -> [(frame, row)], ids in order of first appearance
        for row, (i, f) in enumerate(zip(ids, frames)):
            if i is not None:
                tracks.setdefault(i, []).append((f, row))
        slots, last = dict(self._slots), dict(self._last)
        free = sorted(set(range(self.max_tracks)) - set(slots.values()), reverse=True)
        offsets, rows, gap, slot = [0], [], [], []
        for i, samples in tracks.items():
            samples.sort()
            for (f0, _), (f1, _) in zip(samples, samples[1:]):
                if f0 == f1:
                    raise ValueError('track id %r appears twice in frame %d' % (i, f0))
            if i in last and samples[0][0] <= last[i]:
                raise ValueError('track id %r: frame %d does not come after its last sample (frame %d)' % (i, samples[0][0], last[i]))
            if i not in slots:
                if not free:
                    raise ValueError('more than max_tracks = %d live tracks (id %r); reset(track_id) frees a slot' % (self.max_tracks, i))
                slots[i] = free.pop()
            prev = last.get(i)
            for f, row in samples:
                d = 0 if prev is None else f - prev
                gap.append(d if d <= self.max_gap else 0)                          # unseen for more than max_gap frames: the track restarts
                rows.append(row)
                prev = f
            last[i] = prev
            slot.append(slots[i])
            offsets.append(len(rows))
        rows += [row for row, i in enumerate(ids) if i is None]
        i32 = lambda v: np.asarray(v, dtype=np.int32).reshape(-1)
        return SmoothPlan(i32(offsets), i32(rows), i32(gap), i32(slot), list(tracks), (slots, last, None))

    def plan_clip(self, dets_per_frame, track_ids):
        """``plan`` for a clip call: track_ids mirrors dets_per_frame; frame f of the clip is absolute frame frame_counter + f, and the counter
        advances by the number of frames when the plan runs (a clip without any detection advances it at once)."""
        if len(track_ids) != len(dets_per_frame) or any(len(t) != len(d) for t, d in zip(track_ids, dets_per_frame)):
            raise ValueError('track_ids must mirror dets_per_frame: one id (or None) per detection')
        flat = [i for t in track_ids for i in t]
        frames = [self.frame_counter + f for f, t in enumerate(track_ids) for _ in t]
        p = self.plan(flat, frames)
        p.commit = p.commit[:2] + (self.frame_counter + len(dets_per_frame),)
        if not flat:
            self._commit(p)
        return p

    def _commit(self, plan):
        slots, last, counter = plan.commit
        self._slots, self._last = slots, last
        if counter is not None:
            self.frame_counter = counter

    # ---- device
    def _device_state(self, dev):
        if self._state is None or self._state[0].device != dev:
            S, f32 = self.max_tracks, dict(dtype=torch.float32, device=dev)
            self._state = (torch.zeros(S, L.SMOOTH_ROT, 9, **f32), torch.zeros(S, L.SMOOTH_ROT, 3, **f32), torch.zeros(S, L.SMOOTH_SCALAR, **f32),
                           torch.zeros(S, L.SMOOTH_SCALAR, **f32))
        return self._state

    @torch.no_grad()
    def run(self, vis_dict, plan):
        """the device half: upload the table (one non-blocking copy from pinned memory), one filter launch, two SMPL calls.  Returns a new dictionary
        with the keys of ``vis_dict`` and the smoothed tensors in place; ``self.rotmats`` keeps the smoothed (local, global) rotation matrices."""
        local_pose = vis_dict['local_pose']
        if not local_pose.is_cuda:
            raise RuntimeError('TrackSmoother runs on a HIP device only (no CPU fallback)')
        if local_pose.shape[0] != plan.P:
            raise ValueError('the plan is for %d rows, the result has %d' % (plan.P, local_pose.shape[0]))
        dev = local_pose.device
        state = self._device_state(dev)
        self._commit(plan)
        table = torch.from_numpy(plan.table()).pin_memory().to(dev, non_blocking=True)
        c = lambda k: vis_dict[k].float().contiguous()
        sm = L.track_smooth(c('local_pose'), c('global_pose'), c('pred_cam_t'), c('focal_length'), c('shape'), table, plan.T, plan.n_tracked, state,
                            self.min_cutoff, self.beta, self.d_cutoff)
        smpl = self.model.regressor[0].smpl
        out = dict(vis_dict)
        out.update(local_pose=sm['local_pose'], global_pose=sm['global_pose'], pred_cam_t=sm['cam_t'], focal_length=sm['focal'], shape=sm['shape'],
                   local_smpl_vertices=smpl.run(sm['shape'], sm['local_rotmat']).vertices,
                   smpl_vertices=smpl.run(sm['shape'], sm['global_rotmat']).vertices)
        self.rotmats = (sm['local_rotmat'], sm['global_rotmat'])
        return out

    def smooth(self, vis_dict, track_ids, frame_numbers):
        """the stage on its own: rows of ``vis_dict`` with these track ids (None: untracked) at these absolute frame numbers"""
        return self.run(vis_dict, self.plan(track_ids, frame_numbers))
