"""numpy restatement of the temporal smoothing contract (w-hmr_amd/csrc/smooth.hip, TrackSmoother), written from the definition and independent of
the kernel's helpers: rotation log / exp come from scipy.spatial.transform.Rotation.  TEST INFRASTRUCTURE ONLY.

Time is counted in frames.  A track is the sequence of rows with one track id in frame order; D >= 1 is the integer frame gap to the track's previous
sample, a(f, D) = r / (r + 1) with r = 2 pi f D.

    scalar channel    first sample: xh = x, dxh = 0;  then  dx = (x - xh) / D,  dxh = a(d_cutoff, D) dx + (1 - a(d_cutoff, D)) dxh,
                      f = min_cutoff + beta |dxh|,  xh = a(f, D) x + (1 - a(f, D)) xh
    rotation channel  first sample: Rh = R, wh = 0;  then  v = log(Rh^T R) (angle in [0, pi]),  w = v / D,
                      wh = a(d_cutoff, D) w + (1 - a(d_cutoff, D)) wh,  f = min_cutoff + beta |wh|,  Rh = GramSchmidt(Rh exp(a(f, D) v))

The scalar half is the recurrence of the reference tree's OneEuroFilter built with fps = d_cutoff and called with t_e = D: pinned to
tests/golden/one_euro.npz (tests/test_smooth_cpu.py).  ``dtype``: float64 is the reference; float32 rounds every intermediate to fp32 -- the
difference between the two evaluations is the yardstick of the device test's tolerance."""
import numpy as np
from scipy.spatial.transform import Rotation

ROT_CHANNELS, SCALAR_CHANNELS = 25, 14


def smoothing_factor(cutoff, gap, dtype):
    r = dtype(2 * np.pi) * cutoff * dtype(gap)
    return r / (r + dtype(1))


def scalar_step(x, gap, xh, dxh, min_cutoff, beta, d_cutoff, dtype=np.float64):
    """one sample of every scalar channel: x, xh, dxh arrays of one shape -> (xh, dxh)"""
    x, mc, b, dc = x.astype(dtype), dtype(min_cutoff), dtype(beta), dtype(d_cutoff)
    ad = smoothing_factor(dc, gap, dtype)
    dx = (x - xh) / dtype(gap)
    dxh = ad * dx + (dtype(1) - ad) * dxh
    a = smoothing_factor(mc + b * np.abs(dxh), gap, dtype)
    return (a * x + (dtype(1) - a) * xh).astype(dtype), dxh.astype(dtype)


def smooth_scalars(x, gaps, min_cutoff, beta, d_cutoff, dtype=np.float64):
    """x [n, C] samples of one track, gaps [n - 1] -> filtered [n, C]"""
    xh, dxh = x[0].astype(dtype), np.zeros(x.shape[1:], dtype)
    out = [xh]
    for xk, g in zip(x[1:], gaps):
        xh, dxh = scalar_step(xk, int(g), xh, dxh, min_cutoff, beta, d_cutoff, dtype)
        out.append(xh)
    return np.stack(out)


def rot_exp(v, dtype=np.float64):
    """rotation vectors [..., 3] -> matrices [..., 3, 3]"""
    v = np.asarray(v, dtype=np.float64)
    return Rotation.from_rotvec(v.reshape(-1, 3)).as_matrix().reshape(v.shape[:-1] + (3, 3)).astype(dtype)


def rot_log(R, dtype=np.float64):
    """matrices [..., 3, 3] -> rotation vectors [..., 3], angle in [0, pi]"""
    R = np.asarray(R, dtype=np.float64)
    return Rotation.from_matrix(R.reshape(-1, 3, 3)).as_rotvec().reshape(R.shape[:-2] + (3,)).astype(dtype)


def _normalize(v):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), v.dtype.type(1e-12))


def gram_schmidt(M):
    """the package's unbiased Gram-Schmidt of the columns t1, t2, t3 of M [..., 3, 3]: r1 = n((t2 x t3 + t1) / 2), r2 = n(r2' - (r2' . r1) r1) with
    r2' = (t3 x r1 + t2) / 2, r3 = r1 x r2"""
    two = M.dtype.type(2)
    t1, t2, t3 = M[..., :, 0], M[..., :, 1], M[..., :, 2]
    r1 = _normalize((np.cross(t2, t3) + t1) / two)
    r2 = (np.cross(t3, r1) + t2) / two
    r2 = _normalize(r2 - np.sum(r2 * r1, axis=-1, keepdims=True) * r1)
    return np.stack([r1, r2, np.cross(r1, r2)], axis=-1).astype(M.dtype)


def rotation_step(R, gap, Rh, wh, min_cutoff, beta, d_cutoff, dtype=np.float64):
    """one sample of every rotation channel: R, Rh [J, 3, 3], wh [J, 3] -> (Rh, wh)"""
    mc, b, dc = dtype(min_cutoff), dtype(beta), dtype(d_cutoff)
    v = rot_log(np.swapaxes(Rh, -1, -2) @ R.astype(dtype), dtype)
    ad = smoothing_factor(dc, gap, dtype)
    wh = (ad * (v / dtype(gap)) + (dtype(1) - ad) * wh).astype(dtype)
    f = mc + b * np.sqrt(np.sum(wh * wh, axis=-1, keepdims=True)).astype(dtype)
    a = smoothing_factor(f, gap, dtype)
    return gram_schmidt((Rh @ rot_exp((a * v).astype(dtype), dtype)).astype(dtype)), wh


def smooth_tracks(local_pose, global_pose, cam_t, focal, shape, track_ids, frame_numbers, min_cutoff=0.004, beta=1.0, d_cutoff=1.0, max_gap=30,
                  dtype=np.float64):
    """The whole stage on P rows: local_pose / global_pose [P, 72] angle-axis, cam_t [P, 3], focal [P], shape [P, 10]; track_ids [P] (None: untracked),
    frame_numbers [P].  -> dict(local_rotmat, global_rotmat [P, 24, 3, 3], cam_t, focal, shape) in ``dtype``; an untracked row and the first sample
    of a track carry exp(pose) and their own scalars.  A gap above max_gap restarts the track."""
    P = len(track_ids)
    R_in = np.concatenate([rot_exp(np.asarray(local_pose).reshape(P, 24, 3), dtype), rot_exp(np.asarray(global_pose).reshape(P, 24, 3)[:, :1], dtype)], 1)
    x_in = np.concatenate([np.asarray(cam_t).reshape(P, 3), np.asarray(focal).reshape(P, 1), np.asarray(shape).reshape(P, 10)], 1).astype(dtype)
    R_out, x_out = R_in.copy(), x_in.copy()
    tracks = {}
    for row, (i, f) in enumerate(zip(track_ids, frame_numbers)):
        if i is not None:
            tracks.setdefault(i, []).append((int(f), row))
    for samples in tracks.values():
        samples.sort()
        prev = None
        for f, row in samples:
            gap = 0 if prev is None else f - prev
            if gap == 0 or gap > max_gap:
                Rh, wh, xh, dxh = R_in[row], np.zeros((ROT_CHANNELS, 3), dtype), x_in[row], np.zeros(SCALAR_CHANNELS, dtype)
            else:
                Rh, wh = rotation_step(R_in[row], gap, Rh, wh, min_cutoff, beta, d_cutoff, dtype)
                xh, dxh = scalar_step(x_in[row], gap, xh, dxh, min_cutoff, beta, d_cutoff, dtype)
            R_out[row], x_out[row] = Rh, xh
            prev = f
    return dict(local_rotmat=R_out[:, :24], global_rotmat=np.concatenate([R_out[:, 24:], R_out[:, 1:24]], 1), cam_t=x_out[:, :3], focal=x_out[:, 3],
                shape=x_out[:, 4:])
