"""Mesh overlay renderer of the demo on the device: utils/renderer_cam.py (render_overlay_image / render_image_group, pyrender on OpenGL / EGL) as
demo/tester.py:176-214 uses it, restated on csrc/mesh_render.hip -- an Instinct card has no graphics pipeline.

    r = MeshRenderer(smpl_faces)                                   # once: int32 face table + vertex -> face CSR, copied to each device on first use
    img = r.render(frame_u8, verts, cam_t, focal)                  # uint8 [H, W, 3]: all persons of the frame in one depth buffer
    imgs = r.render(frame_u8, verts, cam_t, focal, per_person=True)  # uint8 [P, H, W, 3]: one person per image, as the reference draws them
    imgs = r.render_clip(frames, verts, cam_t, focal, frame_index)  # a clip: F images, row i drawn into frame frame_index[i]; one call, three launches
    strips = render_clip_groups(frames, cam_t, verts, local_verts, None, focal, frame_index, r)     # render_image_group for every person of the clip

Camera, coverage rule and the shading model (pyrender's shader is third-party: the model is defined by this package, diffuse only) are written out in
csrc/mesh_render.hip and docs/kernels.md.  HIP only: CPU tensors raise RuntimeError, like every other entry point here.
"""
import math

import numpy as np
import torch

from .. import _lib as L

DEFAULT_COLOR = (0.65, 0.74, 0.86)      # a light steel blue chosen for this package (bright enough that the four lights do not clip it to white)


def vertex_face_csr(faces, n_verts):
    """vertex -> face adjacency of an [F, 3] face table: (ptr [V + 1], idx [3 F]) int32; the faces of a vertex in increasing face order (the order the
    kernel sums the face normals in)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    flat = f.reshape(-1)
    order = np.argsort(flat, kind='stable')                              # stable: by face index (flat position // 3) within a vertex
    ptr = np.zeros(n_verts + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=n_verts), out=ptr[1:])
    return ptr.astype(np.int32), (order // 3).astype(np.int32)


class MeshRenderer:
    def __init__(self, faces, color=DEFAULT_COLOR):
        """faces: [F, 3] integer face table (numpy / tensor / list); color: (r, g, b) in 0..1, the material's base colour."""
        f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
        f = np.ascontiguousarray(f.reshape(-1, 3).astype(np.int64))
        if f.size == 0 or f.min() < 0:
            raise ValueError('faces must be a non-empty [F, 3] table of non-negative vertex indices')
        self.n_verts_min = int(f.max()) + 1                                 # every mesh drawn with this table needs at least this many vertices
        self.faces = torch.from_numpy(f.astype(np.int32))
        self.color = tuple(float(c) for c in color)
        assert len(self.color) == 3
        self._host = f
        self._dev = {}

    def _tables(self, device, V):
        key = (device, V)
        t = self._dev.get(key)
        if t is None:
            ptr, idx = vertex_face_csr(self._host, V)
            t = self._dev[key] = (self.faces.to(device), torch.from_numpy(ptr).to(device), torch.from_numpy(idx).to(device))
        return t

    @torch.no_grad()
    def render(self, frame_u8, verts, cam_t, focal, center=None, rot=None, sideview_angle=0, per_person=False, want=(), size=None, znear=0.05):
        """frame_u8: uint8 [H, W, 3] on the device, or None for a black background of ``size`` = (H, W); verts [P, V, 3] in the mesh frame
        (``local_smpl_vertices`` / ``smpl_vertices``), cam_t [P, 3] (``pred_cam_t``), focal [P] or [P, 2] (``focal_length``), all device tensors;
        center (cx, cy), default (W // 2, H // 2) (tester.py:185); rot: camera_rotation as 3 x 3 HOST values (the demo passes the identity,
        tester.py:194) or None; sideview_angle in degrees about Y.  want: any of 'color', 'face', 'depth', 'screen' -> a dict (see _lib.mesh_render).
        Nothing here waits for the device: the call can be captured in a HIP graph or follow a replayed one on the same stream."""
        for t in (frame_u8, verts, cam_t, focal):
            if t is not None and not (torch.is_tensor(t) and t.is_cuda):
                raise RuntimeError('MeshRenderer.render needs HIP device tensors; there is no CPU fallback')
        if frame_u8 is not None:
            H, W = frame_u8.shape[:2]
            frame_u8 = frame_u8.contiguous()
        else:
            H, W = size
        verts = verts.float().contiguous()
        P, V = verts.shape[0], verts.shape[1]
        if V < self.n_verts_min:
            raise ValueError('the face table indexes %d vertices, the mesh has %d' % (self.n_verts_min, V))
        cam_t = cam_t.float().reshape(P, 3).contiguous()
        focal = focal.float().reshape(P, -1)
        focal = (focal.expand(P, 2) if focal.shape[1] == 1 else focal).contiguous()
        if center is None:
            center = (W // 2, H // 2)
        if rot is not None and torch.is_tensor(rot):
            if rot.is_cuda:
                raise RuntimeError('rot is read on the host (it enters the launch as kernel arguments): pass a CPU tensor, numpy array or nested list')
            rot = rot.reshape(3, 3).tolist()
        faces, ptr, idx = self._tables(verts.device, V)
        return L.mesh_render(verts, faces, ptr, idx, cam_t, focal, center, frame_u8, (H, W), self.color, rot=rot, sideview_angle=sideview_angle,
                             per_person=per_person, znear=znear, want=want)

    # ---- draw list: many mesh instances into many images in one call (csrc/mesh_render.hip: whmr_mesh_render_draws)
    def plan_draws(self, sizes, draws, centers=None, frame_strides=None, out_strides=None, have_verts1=False, n_rows=None):
        """The two tables of whmr_mesh_render_draws from what the host knows, before anything is launched.  sizes: (H, W) per target image; draws:
        (row, verts_set, image, sideview_angle in degrees) per mesh instance, in drawing order (an earlier draw wins a depth tie); centers: (cx, cy) per
        image, default (W // 2, H // 2); frame_strides / out_strides: bytes per row of each background / output, default 3 W.  Returns (images, draws,
        total_pixels): numpy records of _lib.RENDER_IMAGE_DTYPE / RENDER_DRAW_DTYPE with ``pix_off`` the running sum of H * W and the ``frame`` / ``out``
        pointers left 0 for the caller.  ValueError: an image index out of range, an image without pixels, a row outside [0, n_rows), a verts_set
        other than 0 or (with have_verts1) 1, n_draws * n_faces >= 2^31, more than 65535 images."""
        sizes = [(int(h), int(w)) for h, w in sizes]
        NI, D, F = len(sizes), len(draws), int(self.faces.shape[0])
        if not 1 <= NI <= 65535:
            raise ValueError('a draw list has 1 .. 65535 target images, got %d' % NI)
        if D * F >= 2 ** 31:
            raise ValueError('%d draws of %d faces: the global face id draw * F + face needs D * F < 2^31' % (D, F))
        images = np.zeros(NI, dtype=L.RENDER_IMAGE_DTYPE)
        for i, (h, w) in enumerate(sizes):
            if h < 1 or w < 1:
                raise ValueError('image %d has no pixels (%d x %d)' % (i, h, w))
        images['H'], images['W'] = [h for h, _ in sizes], [w for _, w in sizes]
        planes = images['H'].astype(np.int64) * images['W']
        images['pix_off'] = np.cumsum(planes) - planes
        if centers is None:
            centers = [(w // 2, h // 2) for h, w in sizes]
        images['cx'], images['cy'] = [float(c[0]) for c in centers], [float(c[1]) for c in centers]
        images['frame_row_stride'] = [3 * w for _, w in sizes] if frame_strides is None else [int(v) for v in frame_strides]
        images['out_row_stride'] = [3 * w for _, w in sizes] if out_strides is None else [int(v) for v in out_strides]
        table = np.zeros(D, dtype=L.RENDER_DRAW_DTYPE)
        for d, (row, vset, img, angle) in enumerate(draws):
            if not 0 <= int(img) < NI:
                raise ValueError('draw %d names image %d of %d' % (d, img, NI))
            if int(row) < 0 or (n_rows is not None and int(row) >= n_rows):
                raise ValueError('draw %d names row %d of %s' % (d, row, n_rows))
            if int(vset) not in ((0, 1) if have_verts1 else (0,)):
                raise ValueError('draw %d: verts_set %d%s' % (d, vset, ' without a second vertex tensor' if int(vset) == 1 else ' (0 or 1)'))
            a = math.radians(float(angle))
            table[d] = (int(row), int(vset), int(img), math.cos(a), math.sin(a), (0, 0, 0))
        return images, table, int(planes.sum())

    def upload_draws(self, images, table, backgrounds, outputs, device):
        """fill in the pointers of the planned tables (backgrounds: per image a uint8 device tensor or None = black; outputs: the tensors written) and
        send both tables up in one non-blocking copy from pinned memory -> (images, draws) as uint8 device tensors.  The caller keeps the
        backgrounds and outputs alive for as long as the tables are drawn with."""
        images['frame'] = [0 if b is None else b.data_ptr() for b in backgrounds]
        images['out'] = [o.data_ptr() for o in outputs]
        n_img = images.nbytes
        host = torch.empty(n_img + table.nbytes, dtype=torch.uint8).pin_memory()
        host.numpy()[:n_img] = images.view(np.uint8)
        host.numpy()[n_img:] = table.view(np.uint8)
        both = host.to(device, non_blocking=True)
        return both[:n_img], both[n_img:]

    @torch.no_grad()
    def run_draws(self, tables, n_images, n_draws, total_pixels, verts0, verts1, cam_t, focal, rot=None, znear=0.05, want=()):
        """the launch group over uploaded tables (``upload_draws``): three launches, no host sync, nothing allocated but the planes asked for in
        ``want`` -- with fixed tables the call can be captured in a HIP graph.  verts0, verts1 (or None) [R, V, 3], cam_t [R, 3], focal [R, 2] fp32,
        contiguous.  -> the dict of _lib.mesh_render_draws."""
        if rot is not None and torch.is_tensor(rot):
            if rot.is_cuda:
                raise RuntimeError('rot is read on the host (it enters the launch as kernel arguments): pass a CPU tensor, numpy array or nested list')
            rot = rot.reshape(3, 3).tolist()
        faces, ptr, idx = self._tables(verts0.device, verts0.shape[1])
        return L.mesh_render_draws(verts0, verts1, faces, ptr, idx, cam_t, focal, tables[1], n_draws, tables[0], n_images, total_pixels, self.color,
                                   rot=rot, znear=znear, want=want)

    def _run_draws(self, images, table, total, backgrounds, outputs, verts0, verts1, cam_t, focal, rot, znear, want):
        tables = self.upload_draws(images, table, backgrounds, outputs, verts0.device)
        return self.run_draws(tables, len(images), len(table), total, verts0, verts1, cam_t, focal, rot=rot, znear=znear, want=want)

    def _rows(self, verts, cam_t, focal, what):
        for t in (verts, cam_t, focal):
            if not (torch.is_tensor(t) and t.is_cuda):
                raise RuntimeError('MeshRenderer.%s needs HIP device tensors; there is no CPU fallback' % what)
        verts = verts.float().contiguous()
        P, V = verts.shape[0], verts.shape[1]
        if V < self.n_verts_min:
            raise ValueError('the face table indexes %d vertices, the mesh has %d' % (self.n_verts_min, V))
        focal = focal.float().reshape(P, -1)
        return verts, cam_t.float().reshape(P, 3).contiguous(), (focal.expand(P, 2) if focal.shape[1] == 1 else focal).contiguous()

    @torch.no_grad()
    def render_clip(self, frames, verts, cam_t, focal, frame_index, per_person=False, centers=None, rot=None, znear=0.05, want=()):
        """The overlays of a clip in ONE call of three launches.  frames: uint8 [F, H, W, 3] on the device or a list of [H_i, W_i, 3] device tensors of
        any sizes and row strides; verts [P, V, 3], cam_t [P, 3], focal [P] or [P, 2]: all persons of the clip; frame_index: the frame of every row
        as HOST integers (list, numpy array, CPU tensor; a device tensor raises RuntimeError: the draw table is packed on the host).  Returns a list
        of F uint8 images [H_i, W_i, 3], all persons of a frame in one depth buffer exactly as ``render`` draws that frame's rows (views of one
        [F, H, W, 3] tensor when the sizes agree; a frame without rows comes back as its own bytes), or with per_person P images, one per row over
        its frame.  centers: (cx, cy) per frame, default (W_i // 2, H_i // 2).  want as for ``render``: a dict with 'image' and lists of per-image
        planes ('face': the global id draw * F + face with draw = the row; 'screen' [P, V, 3]).  No host sync, no read of device memory."""
        if torch.is_tensor(frame_index):
            if frame_index.is_cuda:
                raise RuntimeError('frame_index is read on the host (the draw table is packed there): pass a list, numpy array or CPU tensor')
            frame_index = frame_index.tolist()
        index = [int(i) for i in np.asarray(frame_index).reshape(-1)]
        frame_list = list(frames.unbind(0)) if torch.is_tensor(frames) else list(frames)
        for f in frame_list:
            if not (torch.is_tensor(f) and f.is_cuda):
                raise RuntimeError('MeshRenderer.render_clip needs HIP device tensors; there is no CPU fallback')
            if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3:
                raise ValueError('a frame is uint8 [H, W, 3], got %s %s' % (f.dtype, tuple(f.shape)))
        frame_list = [f if f.stride(2) == 1 and f.stride(1) == 3 else f.contiguous() for f in frame_list]      # rows may be strided, pixels are packed
        verts, cam_t, focal = self._rows(verts, cam_t, focal, 'render_clip')
        P, n_frames = verts.shape[0], len(frame_list)
        if len(index) != P:
            raise ValueError('%d rows but %d frame indices' % (P, len(index)))
        if any(not 0 <= i < n_frames for i in index):
            raise ValueError('frame_index names a frame outside 0 .. %d' % (n_frames - 1))
        if centers is not None and len(centers) != n_frames:
            raise ValueError('%d frames but %d centres' % (n_frames, len(centers)))
        if P == 0:                                                                    # nothing to draw: no image per person, every frame as it is
            images = [] if per_person else [f.clone() for f in frame_list]
            return dict({k: [] for k in want}, image=images) if want else images
        targets = index if per_person else list(range(n_frames))                      # the frame behind every target image
        backgrounds = [frame_list[i] for i in targets]
        sizes = [tuple(b.shape[:2]) for b in backgrounds]
        if len(set(sizes)) == 1:
            outputs = list(torch.empty((len(sizes),) + sizes[0] + (3,), dtype=torch.uint8, device=verts.device).unbind(0))
        else:
            outputs = [torch.empty(s + (3,), dtype=torch.uint8, device=verts.device) for s in sizes]
        draws = [(row, 0, row if per_person else i, 0.0) for row, i in enumerate(index)]
        images, table, total = self.plan_draws(sizes, draws, centers=None if centers is None else [centers[i] for i in targets],
                                               frame_strides=[b.stride(0) for b in backgrounds], n_rows=P)
        res = self._run_draws(images, table, total, backgrounds, outputs, verts, None, cam_t, focal, rot, znear, want)
        if not want:
            return outputs
        out = {'image': outputs}
        for k, plane in res.items():
            out[k] = plane if k == 'screen' else [plane[o:o + h * w].view((h, w) + tuple(plane.shape[1:])) for o, (h, w) in zip(images['pix_off'].tolist(), sizes)]
        return out


def render_overlay_image(image, camera_translation, vertices, camera_rotation, focal_length, camera_center, renderer, sideview_angle=0):
    """renderer_cam.py:41-141 for ONE person: image uint8 [H, W, 3] (device), camera_translation [3], vertices [V, 3], focal_length (fx, fy) or a
    [1] / [2] tensor, camera_center (cx, cy); ``renderer`` replaces the faces / mesh_color arguments.  Returns uint8 [H, W, 3]; unlike the reference,
    camera_translation is not modified in place.  mesh_filename (.obj export) and add_ground_plane are out of scope."""
    if not torch.is_tensor(focal_length):
        focal_length = torch.tensor([float(focal_length[0]), float(focal_length[1])], device=vertices.device)
    return renderer.render(image, vertices.unsqueeze(0), camera_translation.reshape(1, 3), focal_length.reshape(1, -1), center=camera_center,
                           rot=camera_rotation, sideview_angle=sideview_angle)


def render_image_group(image, camera_translation, vertices, local_vertices, camera_rotation, focal_length, camera_center, renderer):
    """renderer_cam.py:144-225: the [H, 4 W, 3] uint8 strip  frame | overlay of local_vertices | side view (270 degrees) of local_vertices | side view
    of vertices,  side views on a black background.  Out of scope: the checkerboard ground plane of the first side view (a PARE helper that is not in
    the reference tree), the keypoint skeleton, .obj export and cv2.imwrite -- the tensor is returned and the caller saves it."""
    over = render_overlay_image(image, camera_translation, local_vertices, camera_rotation, focal_length, camera_center, renderer)
    black = torch.zeros_like(image)
    side0 = render_overlay_image(black, camera_translation, local_vertices, camera_rotation, focal_length, camera_center, renderer, sideview_angle=270)
    side1 = render_overlay_image(black, camera_translation, vertices, camera_rotation, focal_length, camera_center, renderer, sideview_angle=270)
    return torch.cat([image, over, side0, side1], dim=1)


@torch.no_grad()
def render_clip_groups(frames, camera_translation, vertices, local_vertices, camera_rotation, focal_length, frame_index, renderer, camera_centers=None):
    """``render_image_group`` for every person of a clip in ONE call of three launches.  frames: uint8 [F, H, W, 3] or a list of [H_i, W_i, 3] device
    tensors; camera_translation [P, 3], vertices / local_vertices [P, V, 3], focal_length [P] or [P, 2]: all persons of the clip; frame_index: the
    frame of every person as HOST integers; camera_rotation: 3 x 3 HOST values or None; camera_centers: (cx, cy) per frame, default the frame centre.
    Returns P strips uint8 [H_i, 4 W_i, 3] (views of one [P, H, 4 W, 3] tensor when the sizes agree), equal to render_image_group per person: the
    frame is copied into panel 0 and the three draws of a person (local at 0 degrees over the frame, local and vertices at 270 degrees on black) are
    written straight into panels 1 to 3 through the output row stride."""
    if torch.is_tensor(frame_index):
        if frame_index.is_cuda:
            raise RuntimeError('frame_index is read on the host (the draw table is packed there): pass a list, numpy array or CPU tensor')
        frame_index = frame_index.tolist()
    index = [int(i) for i in np.asarray(frame_index).reshape(-1)]
    frame_list = list(frames.unbind(0)) if torch.is_tensor(frames) else list(frames)
    for f in frame_list:
        if not (torch.is_tensor(f) and f.is_cuda):
            raise RuntimeError('render_clip_groups needs HIP device tensors; there is no CPU fallback')
    frame_list = [f if f.stride(2) == 1 and f.stride(1) == 3 else f.contiguous() for f in frame_list]
    local, cam_t, focal = renderer._rows(local_vertices, camera_translation, focal_length, 'render_clip_groups')
    world = vertices.float().contiguous()
    P = local.shape[0]
    if world.shape != local.shape or len(index) != P or P == 0:
        raise ValueError('vertices %s, local_vertices %s and %d frame indices do not describe one set of persons' % (tuple(world.shape), tuple(local.shape), len(index)))
    if any(not 0 <= i < len(frame_list) for i in index):
        raise ValueError('frame_index names a frame outside 0 .. %d' % (len(frame_list) - 1))
    shapes = [tuple(frame_list[i].shape[:2]) for i in index]
    if len(set(shapes)) == 1:
        strips = list(torch.empty(P, shapes[0][0], 4 * shapes[0][1], 3, dtype=torch.uint8, device=local.device).unbind(0))
    else:
        strips = [torch.empty(h, 4 * w, 3, dtype=torch.uint8, device=local.device) for h, w in shapes]
    sizes, centers, backgrounds, outputs, draws = [], [], [], [], []
    for p, (i, (h, w)) in enumerate(zip(index, shapes)):
        for panel, drawn in enumerate((None, (0, 0.0), (0, 270.0), (1, 270.0))):                    # (verts_set, sideview_angle) of the panel's draw
            if drawn is not None:
                draws.append((p, drawn[0], len(sizes), drawn[1]))
            sizes.append((h, w))
            centers.append((w // 2, h // 2) if camera_centers is None else camera_centers[i])
            backgrounds.append(frame_list[i] if panel < 2 else None)
            outputs.append(strips[p][:, panel * w:(panel + 1) * w])
    images, table, total = renderer.plan_draws(sizes, draws, centers=centers, frame_strides=[frame_list[i].stride(0) for i in index for _ in range(4)],
                                               out_strides=[o.stride(0) for o in outputs], have_verts1=True, n_rows=P)
    renderer._run_draws(images, table, total, backgrounds, outputs, local, world, cam_t, focal, camera_rotation, 0.05, ())
    return strips
