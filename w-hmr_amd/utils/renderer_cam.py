"""Mesh overlay renderer of the demo on the device: utils/renderer_cam.py (render_overlay_image / render_image_group, pyrender on OpenGL / EGL) as
demo/tester.py:176-214 uses it, restated on csrc/mesh_render.hip -- an Instinct card has no graphics pipeline.

    r = MeshRenderer(smpl_faces)                                   # once: int32 face table + vertex -> face CSR, copied to each device on first use
    img = r.render(frame_u8, verts, cam_t, focal)                  # uint8 [H, W, 3]: all persons of the frame in one depth buffer
    imgs = r.render(frame_u8, verts, cam_t, focal, per_person=True)  # uint8 [P, H, W, 3]: one person per image, as the reference draws them

Camera, coverage rule and the shading model (pyrender's shader is third-party: the model is defined by this package, diffuse only) are written out in
csrc/mesh_render.hip and docs/kernels.md.  HIP only: CPU tensors raise RuntimeError, like every other entry point here.
"""
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
