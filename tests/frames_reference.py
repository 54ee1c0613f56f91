"""Integer / float64 numpy restatement of whmr_resize_normalize_frames (csrc/frames.hip): Pillow's Image.resize(..., BILINEAR) on an 8-bit RGB image
[3P Pillow ImagingResample: precompute_coeffs, normalize_coeffs_8bpc, the horizontal pass, then the vertical pass], then ToTensor + Normalize.  The
yardstick of tests/test_clip_gpu.py, itself pinned against Pillow by tests/golden/frames.npz (tests/test_clip_cpu.py).  No import of the package or Pillow.
"""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
PRECISION_BITS = 32 - 8 - 2


def resize_target(H, W, s):
    """torchvision Resize(s) on an H x W image: (h, w), the short side becomes s"""
    return (s, int(s * W / H)) if H <= W else (int(s * H / W), s)


def _triangle(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def resample_coeffs(in_size, out_size):
    """per output index: (first tap, number of taps, taps as integers with 22 fractional bits)"""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    lo, n, kk = np.zeros(out_size, dtype=np.int64), np.zeros(out_size, dtype=np.int64), np.zeros((out_size, ksize), dtype=np.int64)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_triangle((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        lo[xx], n[xx] = xmin, xmax
    return lo, n, kk


def _pass(img, lo, n, kk):
    """one resampling pass along axis 1 of img [R, in, 3] uint8 -> [R, out, 3] uint8"""
    out = np.zeros((img.shape[0], len(lo), 3), dtype=np.uint8)
    src = img.astype(np.int64)
    for xx in range(len(lo)):
        acc = np.full((img.shape[0], 3), 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for k in range(n[xx]):
            acc += src[:, lo[xx] + k] * kk[xx, k]
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_bilinear_u8(img, h, w):
    """[H, W, 3] uint8 -> [h, w, 3] uint8; an axis whose size does not change is copied"""
    H, W = img.shape[:2]
    if w != W:
        img = _pass(img, *resample_coeffs(W, w))
    if h != H:
        img = _pass(img.transpose(1, 0, 2), *resample_coeffs(H, h)).transpose(1, 0, 2)
    return np.ascontiguousarray(img)


def normalise(img_u8):
    """[h, w, 3] uint8 -> [3, h, w] fp32: / 255, - mean, / std (ToTensor + Normalize)"""
    x = np.transpose(img_u8.astype(np.float32), (2, 0, 1)) / np.float32(255.0)
    return (x - MEAN[:, None, None]) / STD[:, None, None]
