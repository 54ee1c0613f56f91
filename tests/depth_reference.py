"""Float64 numpy restatement of the depth auxiliary supervision's definitions (docs/kernels.md, "Depth target"): the inverse-depth rasteriser of
``whmr_depth_rasterize`` and the loss of ``whmr_depth_loss``.  TEST INFRASTRUCTURE ONLY.

What it follows: utils/renderer.py:449-533 of the reference (Depth_Renderer), which delegates the rasterisation to pytorch3d (MeshRasterizer with
blur_radius = ln(1e4) 1e-7, faces_per_pixel = 30; the image is 1 / zbuf[..., 0] with the background's -1 mapped to 0), and core/trainer.py:301-317
(depth_losses).  pytorch3d is on no machine of this project: its published naive rasterisation path for blur_radius > 0 is restated here --
PARITY UNPINNED against the real library, pinned by the analytic known answers of tests/test_depth_supv_cpu.py.  The camera is the IUV
renderer's (oracle/raster.py: camera_K, project).
"""
import numpy as np

from oracle import raster as OR

BLUR_RADIUS = np.log(1.0 / 1e-4) * 1e-7          # renderer.py:494, a SQUARED distance in NDC units


def band_px(W):
    """width in pixels of the band outside every edge that still counts as covered: sqrt(blur_radius) NDC units, 1 px = 2 / W (square image)"""
    return np.sqrt(BLUR_RADIUS) * W / 2.0


def _seg_dist2(ax, ay, bx, by, px, py):
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(l2 > 0, np.clip(((px - ax) * dx + (py - ay) * dy) / l2, 0.0, 1.0), 0.0)
    return (px - (ax + s * dx)) ** 2 + (py - (ay + s * dy)) ** 2


def face_terms(v0, v1, v2, px, py, W):
    """one face at the pixel centres (px, py): -> (covered, pz, margin).  ``margin`` (pixels) is how far the centre is from changing its coverage:
    inside, distance to the nearest edge + band; outside, band - distance (negative: not covered)."""
    area = (v2[0] - v0[0]) * (v1[1] - v0[1]) - (v2[1] - v0[1]) * (v1[0] - v0[0])

    def edge(a, c):
        return (px - a[0]) * (c[1] - a[1]) - (py - a[1]) * (c[0] - a[0])
    w0, w1, w2 = edge(v1, v2) / area, edge(v2, v0) / area, edge(v0, v1) / area
    inside = (w0 > 0) & (w1 > 0) & (w2 > 0)
    d2 = np.minimum(_seg_dist2(v0[0], v0[1], v1[0], v1[1], px, py),
                    np.minimum(_seg_dist2(v1[0], v1[1], v2[0], v2[1], px, py), _seg_dist2(v2[0], v2[1], v0[0], v0[1], px, py)))
    band2 = BLUR_RADIUS * 0.25 * W * W
    covered = inside | (d2 < band2)
    with np.errstate(divide='ignore', invalid='ignore'):
        q0, q1, q2 = w0 / v0[2], w1 / v1[2], w2 / v2[2]
        den = q0 + q1 + q2
        b = [np.clip(q / den, 0.0, 1.0) for q in (q0, q1, q2)]                # perspective-correct from the UNclipped screen barycentrics, then clipped
        s = np.maximum(b[0] + b[1] + b[2], 1e-5)
        pz = (b[0] / s) * v0[2] + (b[1] / s) * v1[2] + (b[2] / s) * v2[2]
    margin = np.where(inside, np.sqrt(d2) + np.sqrt(band2), np.sqrt(band2) - np.sqrt(d2))
    return covered, pz, margin


def rasterize_depth(verts, faces, cam, focal=1000.0, orig_size=(224, 224), out_size=(56, 56), scr=None, want_margin=False):
    """-> (inverse depth [B, 1, H, W], face index [B, H, W] (-1 = background)[, margin [B, H, W]]), float64.  ``scr``: screen coordinates
    [B, V, 3] to use instead of the float64 projection (e.g. fp32-rounded ones).  ``margin``: min over the faces of |face margin| (pixels).
    Every (face, pixel of its box) pair of an image goes through ``face_terms`` in one call; the nearest accepting face per pixel is then picked in
    one sort (pixel, depth, face index)."""
    verts, cam = np.asarray(verts, np.float64), np.asarray(cam, np.float64)
    faces = np.asarray(faces, np.int64)
    B = verts.shape[0]
    H, W = out_size
    assert H == W
    if scr is None:
        scr = OR.project(verts, cam, OR.camera_K(focal, orig_size), focal, orig_size, out_size)
    scr = np.asarray(scr, np.float64)
    fid = -np.ones((B, H * W), np.int64)
    zbuf = np.full((B, H * W), np.inf)
    margin = np.full((B, H * W), np.inf)
    eps = 1e-8 * 0.25 * H * W
    grow = band_px(W) + (2.0 if want_margin else 0.0)
    for b in range(B):
        v = [scr[b, faces[:, k]] for k in range(3)]                                     # three [F, 3]
        xs, ys = np.stack([t[:, 0] for t in v]), np.stack([t[:, 1] for t in v])
        with np.errstate(invalid='ignore'):
            seen = (xs.max(0) + grow >= 0) & (ys.max(0) + grow >= 0) & (xs.min(0) - grow <= W) & (ys.min(0) - grow <= H)      # NaN vertices fail too
        area = (v[2][:, 0] - v[0][:, 0]) * (v[1][:, 1] - v[0][:, 1]) - (v[2][:, 1] - v[0][:, 1]) * (v[1][:, 0] - v[0][:, 0])
        seen &= ~(np.abs(area) <= eps)
        idx = np.nonzero(seen)[0]
        x0 = np.maximum(np.floor(xs[:, idx].min(0) - grow - 0.5).astype(np.int64), 0)
        x1 = np.minimum(np.ceil(xs[:, idx].max(0) + grow - 0.5).astype(np.int64), W - 1)
        y0 = np.maximum(np.floor(ys[:, idx].min(0) - grow - 0.5).astype(np.int64), 0)
        y1 = np.minimum(np.ceil(ys[:, idx].max(0) + grow - 0.5).astype(np.int64), H - 1)
        bw, bh = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
        cnt = bw * bh
        if not cnt.sum():
            continue
        rep = np.repeat(np.arange(len(idx)), cnt)                                          # one entry per (face, pixel of its box)
        local = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        px_i, py_i = x0[rep] + local % bw[rep], y0[rep] + local // bw[rep]
        f = idx[rep]
        covered, pz, m = face_terms(*[[t[f, c] for c in range(3)] for t in v], px_i + 0.5, py_i + 0.5, W)
        pix = py_i * W + px_i
        if want_margin:
            np.minimum.at(margin[b], pix, np.abs(m))
        ok = covered & (pz >= 0)
        pix, f, pz = pix[ok], f[ok], pz[ok]
        order = np.lexsort((f, pz, pix))                                                  # per pixel: nearest first, ties by the smaller face index
        win = order[np.unique(pix[order], return_index=True)[1]]
        zbuf[b, pix[win]], fid[b, pix[win]] = pz[win], f[win]
    with np.errstate(divide='ignore'):
        out = np.where(fid >= 0, 1.0 / zbuf, 0.0).reshape(B, 1, H, W)
    fid = fid.reshape(B, H, W)
    return (out, fid, margin.reshape(B, H, W)) if want_margin else (out, fid)


def smooth_l1(d):
    ad = np.abs(d)
    return np.where(ad < 1.0, 0.5 * d * d, ad - 0.5)


def depth_loss(pred, gt, valid, weight):
    """core/trainer.py:301-317 in float64: -> (loss, d loss / d pred).  pred, gt [B, 1, H, W]; valid [B] (bool / 0-1) or None."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    B = pred.shape[0]
    m = np.ones(B, bool) if valid is None else (np.asarray(valid) != 0)
    if not m.any() or not weight > 0:
        return 0.0, np.zeros_like(pred)
    d = (pred - gt) * m[:, None, None, None]
    return smooth_l1(d).sum() / B * weight, np.clip(d, -1.0, 1.0) * m[:, None, None, None] / B * weight


# ---- the known-answer scenes of the tests: 256 x 256 frame -> 128 x 128, camera (s, tx, ty) = (1, 0, 0) ---------------------------------------
ORIG, OUT, FOCAL = (256, 256), (128, 128), 1000.0
CAM = np.array([[1.0, 0.0, 0.0]])
TZ = 2.0 * FOCAL / (ORIG[0] * 1.0 + 1e-9)


def world(u, v, z):
    """the vertex that the camera CAM puts at pixel (u, v) of the 128 x 128 output with view depth z + TZ (inverse of oracle.raster.project)"""
    fx, fy, px, py = OR.camera_K(FOCAL, ORIG)
    zz = z + TZ
    sx, sy = OUT[1] / ORIG[1], OUT[0] / ORIG[0]
    return [((u - 0.5 * OUT[1]) / sx - (px - 0.5 * ORIG[1])) * zz / fx, ((v - 0.5 * OUT[0]) / sy - (py - 0.5 * ORIG[0])) * zz / fy, z]


def screen_barycentrics(tri, px, py):
    """plain screen-space barycentrics of the centres (px, py) in the triangle of three (u, v) pairs"""
    (x0, y0), (x1, y1), (x2, y2) = tri
    den = (y1 - y2) * (x0 - x2) + (x2 - x1) * (y0 - y2)
    w0 = ((y1 - y2) * (px - x2) + (x2 - x1) * (py - y2)) / den
    w1 = ((y2 - y0) * (px - x2) + (x0 - x2) * (py - y2)) / den
    return w0, w1, 1.0 - w0 - w1


TILTED_UV = ((20.0, 20.0), (100.0, 30.0), (40.0, 110.0))
TILTED_Z = (-0.5, 0.0, 0.5)                                                          # vertex depths spread by +-0.5 m


def tilted_triangle():
    """-> (verts [1, 3, 3], faces, interior mask [128, 128], analytic inverse depth sum_i w_i / z_i there)"""
    verts = np.array([[world(u, v, z) for (u, v), z in zip(TILTED_UV, TILTED_Z)]])
    yy, xx = np.mgrid[0:OUT[0], 0:OUT[1]] + 0.5
    w = screen_barycentrics(TILTED_UV, xx, yy)
    interior = (w[0] > 0.01) & (w[1] > 0.01) & (w[2] > 0.01)
    inv = sum(wi / (z + TZ) for wi, z in zip(w, TILTED_Z))
    return verts, np.array([[0, 1, 2]]), interior, inv


EDGE_ROW = 30                                                                         # the pixel row whose centres sit just outside the top edge


def edge_triangle(offset):
    """a triangle whose horizontal top edge lies ``offset`` pixels BELOW the centres of row EDGE_ROW (which are thus outside it, ``offset`` from the
    edge segment for the columns 25..94).  -> (verts, faces, (row, columns), expected inverse depth there by the clamp-and-renormalise rule)"""
    yc = EDGE_ROW + 0.5
    uv = ((20.0, yc + offset), (100.0, yc + offset), (60.0, 100.0))
    zs = (-0.3, 0.4, 0.1)
    verts = np.array([[world(u, v, z) for (u, v), z in zip(uv, zs)]])
    cols = np.arange(25, 95)
    w = screen_barycentrics(uv, cols + 0.5, np.full(cols.shape, yc))                  # w[2] < 0: the centre is beyond the edge opposite vertex 2
    zv = [z + TZ for z in zs]
    q = [wi / zi for wi, zi in zip(w, zv)]
    b = [np.clip(qi / (q[0] + q[1] + q[2]), 0.0, 1.0) for qi in q]
    s = np.maximum(b[0] + b[1] + b[2], 1e-5)
    pz = sum(bi / s * zi for bi, zi in zip(b, zv))
    return verts, np.array([[0, 1, 2]]), (EDGE_ROW, cols), 1.0 / pz


STACK_UV = ((30.0, 25.0), (95.0, 40.0), (50.0, 100.0))


def stacked_triangles():
    """two triangles with one screen footprint, vertices 0..2 at depth 0, vertices 3..5 half a metre nearer -> (verts [1, 6, 3], interior mask)"""
    verts = np.array([[world(u, v, 0.0) for u, v in STACK_UV] + [world(u, v, -0.5) for u, v in STACK_UV]])
    yy, xx = np.mgrid[0:OUT[0], 0:OUT[1]] + 0.5
    w = screen_barycentrics(STACK_UV, xx, yy)
    return verts, (w[0] > 0.01) & (w[1] > 0.01) & (w[2] > 0.01)


def behind_camera_triangle():
    """the footprint of STACK_UV with view depth -2 (behind the camera): culled"""
    return np.array([[world(u, v, -2.0 - TZ) for u, v in STACK_UV]]), np.array([[0, 1, 2]])


def degenerate_triangle():
    """two coincident vertices (area exactly 0 in every precision) and a third, on a line 0.01 px below the centres of row EDGE_ROW: the band around
    that segment would cover them if the area cut did not skip the face"""
    yc = EDGE_ROW + 0.51
    return np.array([[world(20.0, yc, 0.0), world(20.0, yc, 0.0), world(100.0, yc, -0.1)]]), np.array([[0, 1, 2]])
