"""Integer / float32 numpy restatement of the occluder stage of the training-batch maker (stage 4a of csrc/augment.hip, whmr_amd.datasets.train_batch):
the yardstick of tests/test_occlusion_gpu.py.  No import of the package or of the reference.

One paste = (occluder index, factor, cx, cy) on the 256 x 256 uint8 patch after the flip and before the colour noise:
  size   (nw, nh) = np.round((w, h) * factor).astype(int)            (float64, half to even); a zero size drops the paste
  start  np.round((cx, cy)).astype(int32) - (nw, nh) // 2
  resize area average DEFINED in integers: along an axis of source length S resized to n, output u covers [u S, (u + 1) S) and source texel j
         covers [j n, (j + 1) n) in units of 1 / n texel; weight = the integer overlap (an axis' weights sum to S);
         channel = (2 sum(wy wx v) + D) // (2 D), D = w h (round half up), all four channels alike
  blend  a = float32(A) / float32(255); dst = uint8(a * src + (float32(1) - a) * dst), every product and the sum rounded to fp32, truncated
"""
import numpy as np

RES = 256
X0, X1 = 32, 224


def axis_weights(S, n):
    """[n, S] int64: overlap of output u = [u S, (u + 1) S) with source texel j = [j n, (j + 1) n)"""
    u, j = np.arange(n, dtype=np.int64)[:, None], np.arange(S, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((u + 1) * S, (j + 1) * n) - np.maximum(u * S, j * n))


def area_resize_u8(img, nw, nh):
    """[h, w, C] uint8 -> [nh, nw, C] uint8 (1 <= nw <= w, 1 <= nh <= h)"""
    h, w = img.shape[:2]
    assert 1 <= nw <= w and 1 <= nh <= h and img.dtype == np.uint8
    wy, wx = axis_weights(h, nh), axis_weights(w, nw)
    assert (wy.sum(1) == h).all() and (wx.sum(1) == w).all()
    rows = np.tensordot(wy, img.astype(np.int64), axes=(1, 0))                   # [nh, w, C]: sum over y of wy v
    total = np.tensordot(wx, rows, axes=(1, 1)).transpose(1, 0, 2)               # [nh, nw, C]: sum over x of wx (...)
    D = w * h
    return ((2 * total + D) // (2 * D)).astype(np.uint8)


def paste_size(h, w, factor):
    nw, nh = np.round(np.array([w, h]) * factor).astype(int)
    return int(nw), int(nh)


def paste_start(cx, cy, nw, nh):
    c = np.round(np.array([cx, cy])).astype(np.int32)
    s = c - np.array([nw, nh]) // 2
    return int(s[0]), int(s[1])


def paste_over(patch, rgba, sx, sy, x_range=(0, RES)):
    """alpha-blend rgba [nh, nw, 4] into patch [256, W, 3] (uint8, in place) at [start, start + (nw, nh)), clipped to the rows and to the columns
    x_range of the patch"""
    nh, nw = rgba.shape[:2]
    x0, x1, y0, y1 = max(sx, x_range[0]), min(sx + nw, x_range[1]), max(sy, 0), min(sy + nh, patch.shape[0])
    if x1 <= x0 or y1 <= y0:
        return patch
    src = rgba[y0 - sy:y1 - sy, x0 - sx:x1 - sx]
    a = src[..., 3:4].astype(np.float32) / np.float32(255)
    dst = patch[y0:y1, x0:x1].astype(np.float32)
    out = a * src[..., :3].astype(np.float32) + (np.float32(1) - a) * dst
    assert out.dtype == np.float32
    patch[y0:y1, x0:x1] = out.astype(np.uint8)
    return patch


def occlude_patch(patch_u8, occluders, pastes, x_range=(0, RES)):
    """patch_u8 [256, 256, 3] uint8 (after the flip, before pn); pastes: rows (occluder index, factor, cx, cy), applied in order -> a new patch"""
    out = patch_u8.copy()
    for k, factor, cx, cy in np.asarray(pastes, dtype=np.float64).reshape(-1, 4):
        obj = occluders[int(k)]
        nw, nh = paste_size(obj.shape[0], obj.shape[1], factor)
        if nw == 0 or nh == 0:
            continue
        sx, sy = paste_start(cx, cy, nw, nh)
        paste_over(out, area_resize_u8(obj, nw, nh), sx, sy, x_range)
    return out


def rectangles(occluders, pastes):
    """the (index, nw, nh, start_x, start_y) of every paste that is not of zero size, in order"""
    out = []
    for k, factor, cx, cy in np.asarray(pastes, dtype=np.float64).reshape(-1, 4):
        nw, nh = paste_size(occluders[int(k)].shape[0], occluders[int(k)].shape[1], factor)
        if nw and nh:
            out.append((int(k), nw, nh) + paste_start(cx, cy, nw, nh))
    return out
