"""Writes tests/golden/frames.npz: random uint8 frames and what Pillow's Image.resize(..., Image.BILINEAR) makes of them at the size torchvision's
Resize(60) asks for -- the pin of tests/frames_reference.py and of whmr_resize_normalize_frames.  Needs Pillow; the fixture holds arrays only.

    python tests/golden/make_golden_frames.py
"""
import os

import numpy as np
from PIL import Image

S = 60
CASES = {'landscape_down': (75, 100), 'non_integer_ratio': (97, 131), 'portrait_down': (131, 97), 'portrait_up': (40, 30),
         'short_side_unchanged': (60, 83), 'extreme_ratio': (61, 480)}


def resize_target(H, W, s):
    return (s, int(s * W / H)) if H <= W else (int(s * H / W), s)


def pillow_resize(img, s=S):
    h, w = resize_target(img.shape[0], img.shape[1], s)
    return np.asarray(Image.fromarray(img).resize((w, h), Image.BILINEAR))


if __name__ == '__main__':
    rng = np.random.default_rng(11)
    out = {'short_side': np.int64(S), 'pillow_version': np.array(Image.__version__ if hasattr(Image, '__version__') else '')}
    for name, (H, W) in CASES.items():
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        out['in_' + name], out['out_' + name] = img, pillow_resize(img)
    stack = rng.integers(0, 256, size=(3, 97, 131, 3), dtype=np.uint8)
    out['in_stack'], out['out_stack'] = stack, np.stack([pillow_resize(f) for f in stack])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'frames.npz')
    np.savez_compressed(path, **out)
    print(path, {k: v.shape for k, v in out.items()})
