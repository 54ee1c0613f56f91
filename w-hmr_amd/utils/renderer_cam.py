"""Mesh overlay renderer of the demo on the device: utils/renderer_cam.py (render_overlay_image / render_image_group, pyrender on OpenGL / EGL) as
demo/tester.py:176-214 uses it, restated on csrc/mesh_render.hip -- an Instinct card has no graphics pipeline.

    r = MeshRenderer(smpl_faces)                                   # once: int32 face table + vertex -> face CSR, copied to each device on first use
    img = r.render(frame_u8, verts, cam_t, focal)                  # uint8 [H, W, 3]: all persons of the frame in one depth buffer
    imgs = r.render(frame_u8, verts, cam_t, focal, per_person=True)  # uint8 [P, H, W, 3]: one person per image, as the reference draws them
    imgs = r.render_clip(frames, verts, cam_t, focal, frame_index)  # a clip: F images, row i drawn into frame frame_index[i]; one call, three launches
    strips = render_clip_groups(frames, cam_t, verts, local_verts, None, focal, frame_index, r)     # render_image_group for every person of the clip
    imgs = r.render(None, verts, cam_t, focal, size=(H, W), per_person=True, sideview_angle=270, ground=True)     # a checkerboard floor under every person
    export_obj('person_rot.obj', verts[0], smpl_faces, sideview_angle=270)                          # the mesh as the reference's --save_obj writes it
    img = r.render(frame_u8, verts, cam_t, focal, wireframe=True, joints=joints49)                  # hidden-line wireframe over the keypoint skeleton

Camera, coverage rule and the shading model (pyrender's shader is third-party: the model is defined by this package, diffuse only) are written out in
csrc/mesh_render.hip and docs/kernels.md.  HIP only: CPU tensors raise RuntimeError, like every other entry point here.
"""
import math

import numpy as np
import torch

from .. import _lib as L
from ..core import constants as K

DEFAULT_COLOR = (0.65, 0.74, 0.86)      # a light steel blue chosen for this package (bright enough that the four lights do not clip it to white)
# The checkerboard ground plane (csrc/mesh_render.hip): a 4 m square of 9 x 9 tiles.  The tile greys are recalled from PARE's get_checkerboard_plane,
# which is not in the reference tree: unverified, so they are parameters of MeshRenderer.
GROUND_HALF, GROUND_TILES = 2.0, 9
GROUND_DARK, GROUND_LIGHT = 35 / 255, 220 / 255


# Keypoint skeletons and wireframe (csrc/mesh_render.hip: whmr_mesh_render_marked).  The drawing is defined by this package -- the reference draws with
# cv2 through PARE's draw_skeleton, neither in its tree; pixel parity with cv2 is unpinned -- and so are the colours and widths (core/constants.py).
LAYERS = {'under': 0, 'over': 1, 0: 0, 1: 1}


def _marked(wireframe, joints, keypoints_2d, want):
    """do the arguments of a render call ask for the marked form?  A call without them goes through the entries it always used."""
    return bool(wireframe) or joints is not None or keypoints_2d is not None or 'overlay' in want or 'keypoints' in want


def _ground_height(ground):
    """the ``ground`` argument of the render calls -> None (no plane), True (at the mesh's lowest point, found on the device) or a float height"""
    if ground is None or ground is False:
        return None
    return True if ground is True else float(ground)


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
    def __init__(self, faces, color=DEFAULT_COLOR, ground_colors=(GROUND_DARK, GROUND_LIGHT), skeleton=K.SPIN_SKELETON, bone_colors=None,
                 joint_color=K.SKELETON_JOINT_RGB):
        """faces: [F, 3] integer face table (numpy / tensor / list); color: (r, g, b) in 0..1, the material's base colour; ground_colors: (dark, light)
        greys in 0..1 of the ground plane's tiles.  skeleton: [NB, 2] joint pairs, the bones of a keypoint skeleton (default: the 25 of the reference's
        get_spin_skeleton over the 49 joints); bone_colors: [NB, 3] in 0..1, default by the bone's side for the default skeleton (left warm, right
        cold, centre yellow: this package's choice) and the centre colour otherwise; joint_color: (r, g, b) of the joint dots, or [J, 3]."""
        f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
        f = np.ascontiguousarray(f.reshape(-1, 3).astype(np.int64))
        if f.size == 0 or f.min() < 0:
            raise ValueError('faces must be a non-empty [F, 3] table of non-negative vertex indices')
        self.n_verts_min = int(f.max()) + 1                                 # every mesh drawn with this table needs at least this many vertices
        self.faces = torch.from_numpy(f.astype(np.int32))
        self.color = tuple(float(c) for c in color)
        assert len(self.color) == 3
        self.ground_colors = (float(ground_colors[0]), float(ground_colors[1]))
        self._host = f
        self._dev = {}
        b = np.asarray(skeleton, dtype=np.int64).reshape(-1, 2)
        if b.size and b.min() < 0:
            raise ValueError('a bone is a pair of non-negative joint indices')
        self.bones = np.ascontiguousarray(b.astype(np.int32))
        self.n_joints_min = int(b.max()) + 1 if b.size else 1
        if bone_colors is None:
            sides = K.SPIN_BONE_SIDE if [tuple(x) for x in b.tolist()] == [tuple(x) for x in K.SPIN_SKELETON] else 'c' * len(b)
            bone_colors = [K.SKELETON_SIDE_RGB[c] for c in sides]
        self.bone_colors = np.ascontiguousarray(np.asarray(bone_colors, dtype=np.float32).reshape(-1, 3))
        self.joint_color = np.asarray(joint_color, dtype=np.float32)
        if self.bone_colors.shape[0] != len(b) or self.joint_color.shape[-1] != 3:
            raise ValueError('bone_colors is [NB, 3] for the %d bones, joint_color (r, g, b) or [J, 3]' % len(b))
        for c in (self.bone_colors, self.joint_color):
            if c.size and not (np.isfinite(c).all() and c.min() >= 0 and c.max() <= 1):
                raise ValueError('colours are in 0..1')
        self._marks = {}

    def _tables(self, device, V):
        key = (device, V)
        t = self._dev.get(key)
        if t is None:
            ptr, idx = vertex_face_csr(self._host, V)
            t = self._dev[key] = (self.faces.to(device), torch.from_numpy(ptr).to(device), torch.from_numpy(idx).to(device))
        return t

    def _mark_tables(self, device, J):
        """(bones [NB, 2] int32, bone_rgb [NB, 3], joint_rgb [J, 3]) on the device, copied on first use.  Keypoints with fewer joints than the
        skeleton names are drawn all the same: a bone that names a joint they do not have is left out (on the device)."""
        t = self._marks.get((device, J))
        if t is None:
            jc = self.joint_color
            if jc.ndim == 2 and jc.shape[0] != J:
                raise ValueError('joint_color has %d rows, the keypoints have %d joints' % (jc.shape[0], J))
            jc = np.ascontiguousarray(np.broadcast_to(jc.reshape(-1, 3), (J, 3)))
            t = self._marks[(device, J)] = (torch.from_numpy(self.bones).to(device), torch.from_numpy(self.bone_colors).to(device),
                                            torch.from_numpy(jc).to(device))
        return t

    @torch.no_grad()
    def render(self, frame_u8, verts, cam_t, focal, center=None, rot=None, sideview_angle=0, per_person=False, want=(), size=None, znear=0.05,
               ground=False, wireframe=False, line_width=None, joints=None, keypoints_2d=None, keypoints_layer='under', bone_width=None,
               joint_radius=None):
        """frame_u8: uint8 [H, W, 3] on the device, or None for a black background of ``size`` = (H, W); verts [P, V, 3] in the mesh frame
        (``local_smpl_vertices`` / ``smpl_vertices``), cam_t [P, 3] (``pred_cam_t``), focal [P] or [P, 2] (``focal_length``), all device tensors;
        center (cx, cy), default (W // 2, H // 2) (tester.py:185); rot: camera_rotation as 3 x 3 HOST values (the demo passes the identity,
        tester.py:194) or None; sideview_angle in degrees about Y.  want: any of 'color', 'face', 'depth', 'screen' -> a dict (see _lib.mesh_render).
        ground: True puts the checkerboard ground plane (csrc/mesh_render.hip) under every person, at the lowest point of that person's mesh,
        found on the device; a float puts it at that world-frame height (y up).  A plane belongs to one person's camera, so ``ground`` needs
        per_person=True or a single row (ValueError otherwise); the dict then also has 'ground_y' [P] (the heights used, NaN = no plane) and, if
        asked for in ``want``, 'ground' (ix * n + iz of the plane's tile, -1 elsewhere); a plane pixel has -1 in 'face'.
        wireframe: True draws the meshes as hidden-line wireframe, lines ``line_width`` pixels wide (an inner edge is drawn by both its faces).
        joints [P, J, 3] (mesh frame, projected by the row's camera, ``SMPL.joints_from_vertices``) or keypoints_2d [P, J, 2 or 3] = (x, y[, confidence])
        in pixels of the image: every row's keypoint skeleton, keypoints_layer 'under' the meshes (where the reference draws it) or 'over'
        everything; bone_width / joint_radius in pixels.  want then also knows 'overlay' (the blended fp32 colour of every pixel) and 'keypoints'
        [P, J, 3] = (u, v, w), w > 0 where the joint is drawn.  The drawing is defined in csrc/mesh_render.hip; a call without these arguments runs
        the kernels it always ran.
        Nothing here waits for the device: the call can be captured in a HIP graph or follow a replayed one on the same stream."""
        height = _ground_height(ground)
        if height is not None and not per_person and verts.shape[0] != 1:
            raise ValueError('a ground plane belongs to one person: %d rows share the image (per_person=True gives every person an image)' % verts.shape[0])
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
        if _marked(wireframe, joints, keypoints_2d, want):
            return self._render_grounded(frame_u8, verts, cam_t, focal, center, rot, sideview_angle, per_person, want, (int(H), int(W)), znear, height,
                                         marks=dict(wireframe=wireframe, line_width=line_width, joints=joints, keypoints_2d=keypoints_2d,
                                                    layer=keypoints_layer, bone_width=bone_width, joint_radius=joint_radius))
        if height is not None:
            return self._render_grounded(frame_u8, verts, cam_t, focal, center, rot, sideview_angle, per_person, want, (int(H), int(W)), znear, height)
        faces, ptr, idx = self._tables(verts.device, V)
        return L.mesh_render(verts, faces, ptr, idx, cam_t, focal, center, frame_u8, (H, W), self.color, rot=rot, sideview_angle=sideview_angle,
                             per_person=per_person, znear=znear, want=want)

    def _render_grounded(self, frame_u8, verts, cam_t, focal, center, rot, sideview_angle, per_person, want, size, znear, height, marks=None):
        """``render`` with a ground plane: one image and one draw per person through the scene form of the draw list; with ``marks`` (wireframe,
        skeletons) through the marked form, all persons in one image unless per_person"""
        P = verts.shape[0]
        NI = P if (per_person or marks is None) else 1
        out = torch.empty((NI,) + size + (3,), dtype=torch.uint8, device=verts.device)
        draws = [(p, 0, p if NI > 1 else 0, sideview_angle) for p in range(P)]
        images, table, total = self.plan_draws([size] * NI, draws, centers=[center] * NI, n_rows=P)
        grounds = None if height is None else self.plan_grounds(NI, draws, [(d[2], p, None if height is True else height) for p, d in enumerate(draws)])
        extra = {}
        if marks is not None:
            extra = self._plan_marks(marks, draws, NI, [d[2] for d in draws], [sideview_angle] * P, P)
        res = self._run_draws(images, table, total, [frame_u8] * NI, list(out.unbind(0)), verts, None, cam_t, focal, rot, znear, want, grounds=grounds, **extra)
        img = out if per_person else out[0]
        if not want:
            return img
        flat = ('screen', 'ground_y', 'keypoints')
        res = {k: v if k in flat else v.view((NI,) + size + tuple(v.shape[1:])) for k, v in res.items() if k != 'ground_y' or height is not None}
        if not per_person:
            res = {k: v if k in flat else v[0] for k, v in res.items()}
        return dict(res, image=img)

    def _plan_marks(self, marks, draws, n_images, images_of_rows, angles, n_rows, layers=None):
        """the keyword arguments of ``_run_draws`` for the marks of a render call: every draw in the call's style, and one skeleton per row of the
        given joints / keypoints_2d into images_of_rows[row] (a list of images: one skeleton each) in the call's layer (or layers[k] for the k-th
        image of a row)"""
        joints, kp = marks.get('joints'), marks.get('keypoints_2d')
        if joints is not None and kp is not None:
            raise ValueError('give the skeleton as joints (projected here) or as keypoints_2d, not both')
        out = dict(styles=self.plan_styles(len(draws), marks.get('wireframe', False), marks.get('line_width')))
        given = joints if joints is not None else kp
        rows = []
        if given is not None:
            if not (torch.is_tensor(given) and given.is_cuda):
                raise RuntimeError('joints / keypoints_2d are HIP device tensors; there is no CPU fallback')
            if given.dim() != 3 or given.shape[0] != n_rows or given.shape[2] not in ((3,) if joints is not None else (2, 3)):
                raise ValueError('%s is [%d, J, %s], got %s' % ('joints' if joints is not None else 'keypoints_2d', n_rows,
                                                                 '3' if joints is not None else '2 or 3', tuple(given.shape)))
            given = given.float()
            if given.shape[2] == 2:
                given = torch.cat([given, torch.ones_like(given[..., :1])], dim=2)
            out['joints' if joints is not None else 'keypoints'] = given.contiguous()
            for row in range(n_rows):
                targets = images_of_rows[row] if isinstance(images_of_rows[row], (list, tuple)) else [images_of_rows[row]]
                for k, img in enumerate(targets):
                    rows.append((row, img, 0 if joints is not None else 1, marks.get('layer', 'under') if layers is None else layers[k], angles[row]))
        out['skeletons'] = self.plan_skeletons(n_images, rows, n_rows=n_rows, bone_width=marks.get('bone_width'), joint_radius=marks.get('joint_radius'))
        return out

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

    def plan_grounds(self, n_images, draws, grounds, half=GROUND_HALF, n=GROUND_TILES):
        """The third table of whmr_mesh_render_scene, one row per image, from what the host knows.  draws: the draw list given to ``plan_draws``;
        grounds: per plane (image, draw, height) or (image, draw, height, half, n) -- the plane of ``image`` belongs to ``draw`` (index into
        ``draws``), which gives its camera and, with height None, its height (the lowest point of the draw's mesh, found on the device); half: half
        the side of the square in metres, n: tiles per side.  Returns numpy records of _lib.RENDER_GROUND_DTYPE (draw = -1: no plane) with this
        renderer's ground_colors.  ValueError: an image or draw index out of range, two planes on one image, a plane whose draw targets another
        image, a plane on an image that several draws share (a plane has one camera), n < 1, half <= 0."""
        n_images = int(n_images)
        table = np.zeros(n_images, dtype=L.RENDER_GROUND_DTYPE)
        table['draw'] = -1
        per_image = np.bincount([int(d[2]) for d in draws if 0 <= int(d[2]) < n_images], minlength=n_images)
        for g in grounds:
            img, d, height = int(g[0]), int(g[1]), g[2]
            g_half, g_n = (float(g[3]), int(g[4])) if len(g) > 3 else (float(half), int(n))
            if not 0 <= img < n_images:
                raise ValueError('a ground plane names image %d of %d' % (img, n_images))
            if not 0 <= d < len(draws):
                raise ValueError('the ground plane of image %d names draw %d of %d' % (img, d, len(draws)))
            if table['draw'][img] >= 0:
                raise ValueError('image %d has two ground planes' % img)
            if int(draws[d][2]) != img:
                raise ValueError('the ground plane of image %d belongs to draw %d, which targets image %d' % (img, d, int(draws[d][2])))
            if per_image[img] != 1:
                raise ValueError('image %d is shared by %d draws: a ground plane belongs to the camera of one' % (img, per_image[img]))
            if g_n < 1 or not g_half > 0:
                raise ValueError('a ground plane has n >= 1 tiles per side and half > 0, got n = %d, half = %g' % (g_n, g_half))
            table[img] = (d, 0 if height is None else 1, 0.0 if height is None else float(height), g_half, g_n, self.ground_colors[0],
                          self.ground_colors[1], 0)
        return table

    def plan_styles(self, n_draws, wireframe=False, line_width=None):
        """The style table of whmr_mesh_render_marked, one row per draw.  wireframe: one bool for all draws or one per draw; line_width: the width
        of a wireframe line in pixels (one for all or one per draw), default core.constants.WIREFRAME_LINE_WIDTH -- half of it enters the table, and
        an inner edge, drawn by both its faces, comes out twice as wide as a silhouette edge.  Returns numpy records of _lib.RENDER_STYLE_DTYPE.
        ValueError: a list of another length than n_draws, a width that is negative or not a number."""
        n_draws = int(n_draws)
        wire = [bool(wireframe)] * n_draws if isinstance(wireframe, (bool, int, np.bool_)) else [bool(w) for w in wireframe]
        width = K.WIREFRAME_LINE_WIDTH if line_width is None else line_width
        width = [float(width)] * n_draws if np.ndim(width) == 0 else [float(w) for w in width]
        if len(wire) != n_draws or len(width) != n_draws:
            raise ValueError('%d draws, but %d wireframe flags and %d line widths' % (n_draws, len(wire), len(width)))
        if any(not (w >= 0 and math.isfinite(w)) for w in width):
            raise ValueError('a line width is a number of pixels >= 0, got %s' % width)
        table = np.zeros(n_draws, dtype=L.RENDER_STYLE_DTYPE)
        table['mode'], table['half_width'] = [int(w) for w in wire], [0.5 * w for w in width]
        return table

    def plan_skeletons(self, n_images, skeletons, n_rows=None, bone_width=None, joint_radius=None):
        """The skeleton table of whmr_mesh_render_marked.  skeletons: per skeleton drawn (row, image, source, layer, sideview_angle in degrees) or
        (..., bone_width, joint_radius): the keypoints of ``row``, drawn into ``image``; source 0 projects the row's 3-D joints with the row's camera
        (and the side rotation), 1 takes its 2-D keypoints; layer 'under' (0) the meshes or 'over' (1) everything; within a layer the skeletons are
        drawn in table order.  bone_width (the whole width of a bone) / joint_radius in pixels, default core.constants.SKELETON_BONE_WIDTH /
        SKELETON_JOINT_RADIUS.  Returns numpy records of _lib.RENDER_SKELETON_DTYPE.  ValueError: an image outside [0, n_images), a row outside
        [0, n_rows), a source other than 0 or 1, a layer other than 'under' / 'over' / 0 / 1, a width or radius that is negative or not a number."""
        n_images = int(n_images)
        table = np.zeros(len(skeletons), dtype=L.RENDER_SKELETON_DTYPE)
        for k, sk in enumerate(skeletons):
            row, img, source, layer, angle = int(sk[0]), int(sk[1]), sk[2], sk[3], float(sk[4])
            width = sk[5] if len(sk) > 5 and sk[5] is not None else (K.SKELETON_BONE_WIDTH if bone_width is None else bone_width)
            radius = sk[6] if len(sk) > 6 and sk[6] is not None else (K.SKELETON_JOINT_RADIUS if joint_radius is None else joint_radius)
            if not 0 <= img < n_images:
                raise ValueError('skeleton %d names image %d of %d' % (k, img, n_images))
            if row < 0 or (n_rows is not None and row >= n_rows):
                raise ValueError('skeleton %d names row %d of %s' % (k, row, n_rows))
            if source not in (0, 1):
                raise ValueError('skeleton %d: source %r (0: the 3-D joints, 1: the 2-D keypoints)' % (k, source))
            if isinstance(layer, (bool, float)) or layer not in LAYERS:
                raise ValueError("skeleton %d: layer %r ('under' or 'over')" % (k, layer))
            width, radius = float(width), float(radius)
            if not (width >= 0 and math.isfinite(width) and radius >= 0 and math.isfinite(radius)):
                raise ValueError('skeleton %d: bone width %g, joint radius %g (pixels, >= 0)' % (k, width, radius))
            a = math.radians(angle)
            table[k] = (row, img, int(source), LAYERS[layer], math.cos(a), math.sin(a), 0.5 * width, radius)
        return table

    def upload_draws(self, images, table, backgrounds, outputs, device, grounds=None, styles=None, skeletons=None):
        """fill in the pointers of the planned tables (backgrounds: per image a uint8 device tensor or None = black; outputs: the tensors written) and
        send the tables up in one non-blocking copy from pinned memory -> (images, draws) as uint8 device tensors, or (images, draws, grounds) with
        the table of ``plan_grounds``, or with ``plan_styles`` / ``plan_skeletons`` tables (either may be None: all solid / no skeleton) the five
        tables (images, draws, grounds, styles, skeletons) of the marked form.  The caller keeps the backgrounds and outputs alive for as long as
        the tables are drawn with."""
        images['frame'] = [0 if b is None else b.data_ptr() for b in backgrounds]
        images['out'] = [o.data_ptr() for o in outputs]
        if styles is not None or skeletons is not None:
            if grounds is None:
                grounds = np.zeros(len(images), dtype=L.RENDER_GROUND_DTYPE)
                grounds['draw'] = -1
            styles = self.plan_styles(len(table)) if styles is None else styles
            skeletons = np.zeros(0, dtype=L.RENDER_SKELETON_DTYPE) if skeletons is None else skeletons
            if len(styles) != len(table):
                raise ValueError('%d draws but %d styles' % (len(table), len(styles)))
            parts = [images, table, grounds, styles, skeletons]
            ends = np.cumsum([t.nbytes for t in parts]).tolist()
            host = torch.empty(ends[-1], dtype=torch.uint8).pin_memory()
            for t, a, b in zip(parts, [0] + ends[:-1], ends):
                host.numpy()[a:b] = t.view(np.uint8)
            up = host.to(device, non_blocking=True)
            return tuple(up[a:b] for a, b in zip([0] + ends[:-1], ends))
        n_img, n_draw = images.nbytes, images.nbytes + table.nbytes
        host = torch.empty(n_draw + (0 if grounds is None else grounds.nbytes), dtype=torch.uint8).pin_memory()
        host.numpy()[:n_img] = images.view(np.uint8)
        host.numpy()[n_img:n_draw] = table.view(np.uint8)
        if grounds is None:
            both = host.to(device, non_blocking=True)
            return both[:n_img], both[n_img:]
        host.numpy()[n_draw:] = grounds.view(np.uint8)
        up = host.to(device, non_blocking=True)
        return up[:n_img], up[n_img:n_draw], up[n_draw:]

    @torch.no_grad()
    def run_draws(self, tables, n_images, n_draws, total_pixels, verts0, verts1, cam_t, focal, rot=None, znear=0.05, want=(), joints=None, keypoints=None):
        """the launch group over uploaded tables (``upload_draws``): three launches, no host sync, nothing allocated but the planes asked for in
        ``want`` -- with fixed tables the call can be captured in a HIP graph.  verts0, verts1 (or None) [R, V, 3], cam_t [R, 3], focal [R, 2] fp32,
        contiguous.  -> the dict of _lib.mesh_render_draws; with a third table (``upload_draws(..., grounds=)``) the scene form draws the ground
        planes in the same launches -> the dict of _lib.mesh_render_scene; with five tables (``upload_draws(..., styles=, skeletons=)``) the marked
        form draws wireframe and the skeletons of joints [R, J, 3] (mesh frame) / keypoints [R, J, 3] = (x, y, confidence), fp32 and contiguous,
        in the same launches -> the dict of _lib.mesh_render_marked."""
        if rot is not None and torch.is_tensor(rot):
            if rot.is_cuda:
                raise RuntimeError('rot is read on the host (it enters the launch as kernel arguments): pass a CPU tensor, numpy array or nested list')
            rot = rot.reshape(3, 3).tolist()
        faces, ptr, idx = self._tables(verts0.device, verts0.shape[1])
        if len(tables) == 5:
            n_skel = tables[4].numel() // L.RENDER_SKELETON_DTYPE.itemsize
            given = joints if joints is not None else keypoints
            if n_skel and given is None:
                raise ValueError('%d skeletons but neither joints nor keypoints' % n_skel)
            bones, bone_rgb, joint_rgb = self._mark_tables(verts0.device, given.shape[1] if given is not None else self.n_joints_min)
            return L.mesh_render_marked(verts0, verts1, faces, ptr, idx, cam_t, focal, tables[1], n_draws, tables[0], n_images, total_pixels, tables[2],
                                        tables[3], tables[4], n_skel, bones, bone_rgb, joint_rgb, joints, keypoints, self.color, rot=rot, znear=znear,
                                        want=want)
        if len(tables) == 3:
            return L.mesh_render_scene(verts0, verts1, faces, ptr, idx, cam_t, focal, tables[1], n_draws, tables[0], n_images, total_pixels, tables[2],
                                       self.color, rot=rot, znear=znear, want=want)
        return L.mesh_render_draws(verts0, verts1, faces, ptr, idx, cam_t, focal, tables[1], n_draws, tables[0], n_images, total_pixels, self.color,
                                   rot=rot, znear=znear, want=want)

    def _run_draws(self, images, table, total, backgrounds, outputs, verts0, verts1, cam_t, focal, rot, znear, want, grounds=None, styles=None,
                   skeletons=None, joints=None, keypoints=None):
        tables = self.upload_draws(images, table, backgrounds, outputs, verts0.device, grounds=grounds, styles=styles, skeletons=skeletons)
        return self.run_draws(tables, len(images), len(table), total, verts0, verts1, cam_t, focal, rot=rot, znear=znear, want=want, joints=joints,
                              keypoints=keypoints)

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
    def render_clip(self, frames, verts, cam_t, focal, frame_index, per_person=False, centers=None, rot=None, znear=0.05, want=(), ground=False,
                    wireframe=False, line_width=None, joints=None, keypoints_2d=None, keypoints_layer='under', bone_width=None, joint_radius=None):
        """The overlays of a clip in ONE call of three launches.  frames: uint8 [F, H, W, 3] on the device or a list of [H_i, W_i, 3] device tensors of
        any sizes and row strides; verts [P, V, 3], cam_t [P, 3], focal [P] or [P, 2]: all persons of the clip; frame_index: the frame of every row
        as HOST integers (list, numpy array, CPU tensor; a device tensor raises RuntimeError: the draw table is packed on the host).  Returns a list
        of F uint8 images [H_i, W_i, 3], all persons of a frame in one depth buffer exactly as ``render`` draws that frame's rows (views of one
        [F, H, W, 3] tensor when the sizes agree; a frame without rows comes back as its own bytes), or with per_person P images, one per row over
        its frame.  centers: (cx, cy) per frame, default (W_i // 2, H_i // 2).  want as for ``render``: a dict with 'image' and lists of per-image
        planes ('face': the global id draw * F + face with draw = the row; 'screen' [P, V, 3]).  ground as for ``render``: a plane under every
        person (per_person=True or a single row, ValueError otherwise), in the same launches; the dict then has 'ground_y' [P].  wireframe,
        line_width, joints / keypoints_2d [P, J, .], keypoints_layer, bone_width, joint_radius and the 'overlay' / 'keypoints' of want as for
        ``render``: every row's skeleton goes into the image its mesh goes into, in the same launches.  No host sync, no read of device memory."""
        height = _ground_height(ground)
        if height is not None and not per_person and verts.shape[0] > 1:
            raise ValueError('a ground plane belongs to one person: %d rows may share an image (per_person=True gives every person an image)' % verts.shape[0])
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
        grounds = None if height is None else self.plan_grounds(len(sizes), draws, [(d[2], row, None if height is True else height) for row, d in enumerate(draws)])
        extra = {}
        if _marked(wireframe, joints, keypoints_2d, want):
            extra = self._plan_marks(dict(wireframe=wireframe, line_width=line_width, joints=joints, keypoints_2d=keypoints_2d, layer=keypoints_layer,
                                          bone_width=bone_width, joint_radius=joint_radius), draws, len(sizes), [d[2] for d in draws], [0.0] * P, P)
        res = self._run_draws(images, table, total, backgrounds, outputs, verts, None, cam_t, focal, rot, znear, want, grounds=grounds, **extra)
        if not want:
            return outputs
        out = {'image': outputs}
        for k, plane in res.items():
            if k == 'ground_y' and height is None:
                continue
            out[k] = plane if k in ('screen', 'ground_y', 'keypoints') else [plane[o:o + h * w].view((h, w) + tuple(plane.shape[1:])) for o, (h, w) in zip(images['pix_off'].tolist(), sizes)]
        return out


def render_overlay_image(image, camera_translation, vertices, camera_rotation, focal_length, camera_center, renderer, sideview_angle=0,
                         add_ground_plane=False, wireframe=False, line_width=None, joints=None, keypoints_2d=None, keypoints_layer='under',
                         bone_width=None, joint_radius=None):
    """renderer_cam.py:41-141 for ONE person: image uint8 [H, W, 3] (device), camera_translation [3], vertices [V, 3], focal_length (fx, fy) or a
    [1] / [2] tensor, camera_center (cx, cy); ``renderer`` replaces the faces / mesh_color arguments.  Returns uint8 [H, W, 3]; unlike the reference,
    camera_translation is not modified in place.  add_ground_plane: True draws the checkerboard floor at the mesh's lowest point (:95-104), a float
    at that height; the default is False where the reference's is True, because the callers of this package have never been given a plane and keep
    their bytes.  mesh_filename is ``export_obj``, a call of its own.  wireframe / line_width, joints [J, 3] or keypoints_2d [J, 2 or 3] with
    keypoints_layer, bone_width, joint_radius: as ``MeshRenderer.render`` (the reference draws the skeleton onto the frame before this call, :165-166:
    here it is one more argument of it)."""
    if not torch.is_tensor(focal_length):
        focal_length = torch.tensor([float(focal_length[0]), float(focal_length[1])], device=vertices.device)
    return renderer.render(image, vertices.unsqueeze(0), camera_translation.reshape(1, 3), focal_length.reshape(1, -1), center=camera_center,
                           rot=camera_rotation, sideview_angle=sideview_angle, ground=add_ground_plane, wireframe=wireframe, line_width=line_width,
                           joints=None if joints is None else joints.unsqueeze(0), keypoints_2d=None if keypoints_2d is None else keypoints_2d.unsqueeze(0),
                           keypoints_layer=keypoints_layer, bone_width=bone_width, joint_radius=joint_radius)


def render_image_group(image, camera_translation, vertices, local_vertices, camera_rotation, focal_length, camera_center, renderer, ground=False,
                       wireframe=False, line_width=None, joints=None, keypoints_2d=None, keypoints_layer='under', bone_width=None, joint_radius=None):
    """renderer_cam.py:144-225: the [H, 4 W, 3] uint8 strip  frame | overlay of local_vertices | side view (270 degrees) of local_vertices | side view
    of vertices,  side views on a black background.  ground=True puts the checkerboard floor of the reference under BOTH side views, each at the
    lowest point of its own mesh (the overlay never has one, :185): against the level floor the camera-frame mesh leans by the camera's pitch and
    roll and the world-frame mesh stands upright.  keypoints_2d [J, 2 or 3] (:157) or joints [J, 3] (mesh frame of local_vertices): the keypoint
    skeleton where the reference puts it (:165-166 draws it onto the frame before anything else) -- on panel 0 and, in ``keypoints_layer``, under
    (or over) the mesh of panel 1; the side views carry none.  wireframe / line_width: the three meshes as hidden-line wireframe.  With any of these
    the strip is one launch group (``render_clip_groups`` of one person).  Out of scope: cv2.imwrite -- the tensor is returned and the caller saves
    it; ``export_obj`` writes the meshes."""
    if _marked(wireframe, joints, keypoints_2d, ()):
        if not torch.is_tensor(focal_length):
            focal_length = torch.tensor([float(focal_length[0]), float(focal_length[1])], device=vertices.device)
        return render_clip_groups([image], camera_translation.reshape(1, 3), vertices.unsqueeze(0), local_vertices.unsqueeze(0), camera_rotation,
                                  focal_length.reshape(1, -1), [0], renderer, camera_centers=[camera_center], ground=ground, wireframe=wireframe,
                                  line_width=line_width, joints=None if joints is None else joints.unsqueeze(0),
                                  keypoints_2d=None if keypoints_2d is None else keypoints_2d.unsqueeze(0), keypoints_layer=keypoints_layer,
                                  bone_width=bone_width, joint_radius=joint_radius)[0]
    over = render_overlay_image(image, camera_translation, local_vertices, camera_rotation, focal_length, camera_center, renderer)
    black = torch.zeros_like(image)
    side0 = render_overlay_image(black, camera_translation, local_vertices, camera_rotation, focal_length, camera_center, renderer, sideview_angle=270,
                                 add_ground_plane=ground)
    side1 = render_overlay_image(black, camera_translation, vertices, camera_rotation, focal_length, camera_center, renderer, sideview_angle=270,
                                 add_ground_plane=ground)
    return torch.cat([image, over, side0, side1], dim=1)


def export_obj(path, vertices, faces, sideview_angle=0, camera_translation=None):
    """The mesh as the reference exports it behind --save_obj (renderer_cam.py:73-87: ``mesh.export(mesh_filename)`` after the 180 degree turn about X
    and, for sideview_angle > 0, the turn about Y): ``v x y z`` lines (%.9g of the float32 coordinates, which reads back exactly) and 1-based
    ``f i j k`` lines -- trimesh's own text is unpinned, the file is defined here.  If ``path`` does not end in ``_rot.obj``, path[:-4] + '.npy'
    gets the camera translation t' = (-t_x, t_y, t_z) (:84-87).  vertices [V, 3] and camera_translation [3] may be device tensors: each is copied
    to the host once."""
    v = (vertices.detach().cpu().numpy() if torch.is_tensor(vertices) else np.asarray(vertices)).astype(np.float64).reshape(-1, 3)
    f = (faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int64).reshape(-1, 3)
    v = v * np.array([1.0, -1.0, -1.0])                                               # D
    if sideview_angle > 0:
        a = math.radians(float(sideview_angle))
        v = v @ np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]]).T       # S
    v = v.astype(np.float32)
    with open(path, 'w') as out:
        out.write(''.join('v %.9g %.9g %.9g\n' % (x, y, z) for x, y, z in v.tolist()))
        out.write(''.join('f %d %d %d\n' % (i + 1, j + 1, k + 1) for i, j, k in f.tolist()))
    if not str(path).endswith('_rot.obj'):
        if camera_translation is None:
            raise ValueError('%s: the camera translation is saved beside every mesh that is not a _rot.obj' % path)
        t = camera_translation.detach().cpu().numpy() if torch.is_tensor(camera_translation) else np.asarray(camera_translation)
        np.save(str(path)[:-4] + '.npy', t.reshape(3) * np.array([-1, 1, 1], dtype=t.dtype))


@torch.no_grad()
def render_clip_groups(frames, camera_translation, vertices, local_vertices, camera_rotation, focal_length, frame_index, renderer, camera_centers=None,
                       ground=False, wireframe=False, line_width=None, joints=None, keypoints_2d=None, keypoints_layer='under', bone_width=None,
                       joint_radius=None):
    """``render_image_group`` for every person of a clip in ONE call of three launches.  frames: uint8 [F, H, W, 3] or a list of [H_i, W_i, 3] device
    tensors; camera_translation [P, 3], vertices / local_vertices [P, V, 3], focal_length [P] or [P, 2]: all persons of the clip; frame_index: the
    frame of every person as HOST integers; camera_rotation: 3 x 3 HOST values or None; camera_centers: (cx, cy) per frame, default the frame centre.
    Returns P strips uint8 [H_i, 4 W_i, 3] (views of one [P, H, 4 W, 3] tensor when the sizes agree), equal to render_image_group per person: the
    frame is copied into panel 0 and the three draws of a person (local at 0 degrees over the frame, local and vertices at 270 degrees on black) are
    written straight into panels 1 to 3 through the output row stride.  ground as for ``render_image_group``: the floor under panels 2 and 3, each
    at its own mesh's lowest point (or at a float height), in the same launch group.  wireframe, line_width, joints / keypoints_2d [P, J, .],
    keypoints_layer, bone_width, joint_radius as for ``render_image_group``: every person's skeleton on panel 0 and under (or over) the mesh of
    panel 1, in the same launch group."""
    height = _ground_height(ground)
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
    grounds = None
    if height is not None:                                                                          # person p: images 4 p + 2, 4 p + 3 are drawn by draws 3 p + 1, 3 p + 2
        y = None if height is True else height
        grounds = renderer.plan_grounds(len(sizes), draws, [(4 * p + k + 1, 3 * p + k, y) for p in range(P) for k in (1, 2)])
    extra = {}
    if _marked(wireframe, joints, keypoints_2d, ()):                                                # person p: the skeleton into images 4 p (the frame) and 4 p + 1
        extra = renderer._plan_marks(dict(wireframe=wireframe, line_width=line_width, joints=joints, keypoints_2d=keypoints_2d, bone_width=bone_width,
                                          joint_radius=joint_radius), draws, len(sizes), [(4 * p, 4 * p + 1) for p in range(P)], [0.0] * P, P,
                                     layers=('under', keypoints_layer))
    renderer._run_draws(images, table, total, backgrounds, outputs, local, world, cam_t, focal, camera_rotation, 0.05, (), grounds=grounds, **extra)
    return strips
