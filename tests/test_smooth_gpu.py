"""Temporal smoothing on the device: whmr_track_smooth / TrackSmoother against the float64 restatement (tests/smooth_reference.py), orthonormality
of a long streamed track, streaming against one call, the two limits of the filter, consistency of the recomputed vertices, and the stage inside
infer_clip / ClipPipeline.

Tolerance of the kernel test (test_kernel_equals_the_float64_reference): the restatement is evaluated once in float32 and once in float64 on the test's
own inputs; the gate is 4x the largest element-wise difference between the two (the device's sin / cos / rsqrt and another order of operations),
and has to come out below the project's 1e-4 gate.  Measured (the restatement needs no device): the float32 evaluation is 2.62e-7 off float64 on the
rotation matrices, 1.75e-7 / 1.99e-7 on the local / global poses compared as rotations, 4.1e-8 / 2.0e-8 / 4.1e-8 on cam_t / focal / shape, so the
gate is 4 x 2.62e-7 = 1.05e-6.  On the MI355X the kernel is 2.4e-7 / 3.0e-7 (rotation matrices), 5.3e-7 / 6.9e-7 (poses) and
the restatement's own 4.1e-8 / 2.0e-8 / 4.1e-8 (scalars) off float64."""
import numpy as np
import pytest
import torch

import smooth_reference as SR
from conftest import ew_err

pytestmark = pytest.mark.gpu
GATE = 1e-4                                          # the project's element-wise parity gate (tests/test_hotpath_gpu.py)
PARAMS = dict(min_cutoff=0.004, beta=1.0, d_cutoff=1.0)
KEYS = ('local_pose', 'global_pose', 'pred_cam_t', 'focal_length', 'shape', 'local_smpl_vertices', 'smpl_vertices')


@pytest.fixture(scope='module')
def model(dev, assets, state_dict):
    from whmr_amd.models import whmr_net
    m = whmr_net(None, assets=assets, numerics='fp32')
    m.load_state_dict(state_dict, strict=False)
    return m.to(dev).eval()


def _tracks_case():
    """6 frames, 3 tracks: 'a' in every frame, 'b' with a two-frame hole (frames 0, 1, 4, 5), 'c' a single sample (frame 2); one untracked row
    (frame 3).  Rows in frame order.  Joint 5 nearly static (1e-4 rad between samples), joint 7 steps by 3.0 rad, the root (local and global) stays
    within 0.05 rad of pi about x."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(17)
    ids = ['a', 'b', 'a', 'b', 'a', 'c', 'a', None, 'a', 'b', 'a', 'b']
    frames = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    P = len(ids)
    base = {i: rng.normal(0, 0.3, size=(24, 3)) for i in ('a', 'b', 'c', None)}
    local, groot = np.zeros((P, 24, 3)), np.zeros((P, 3))
    flip = Rotation.from_rotvec([np.pi, 0.0, 0.0])
    for r, (i, f) in enumerate(zip(ids, frames)):
        local[r] = base[i] + 0.15 * np.sin(0.7 * f + np.arange(24))[:, None] + rng.normal(0, 0.02, size=(24, 3))
        local[r, 5] = base[i][5] + np.array([1e-4 * f, 0.0, 0.0])
        local[r, 7] = np.array([0.1 + (3.0 if f >= 2 else 0.0), 0.0, 0.0])
        local[r, 0] = (flip * Rotation.from_rotvec(rng.uniform(-0.028, 0.028, size=3))).as_rotvec()
        groot[r] = (flip * Rotation.from_rotvec(rng.uniform(-0.028, 0.028, size=3))).as_rotvec()
    local = local.reshape(P, 72).astype(np.float32)
    glob = np.concatenate([groot.astype(np.float32), local[:, 3:]], 1)
    cam_t = (np.array([0.1, 0.2, 5.0]) + np.cumsum(rng.normal(0, 0.05, size=(P, 3)), 0)).astype(np.float32)
    focal = (1000.0 + rng.normal(0, 20.0, size=P)).astype(np.float32)
    shape = (rng.normal(0, 0.5, size=(1, 10)) + rng.normal(0, 0.1, size=(P, 10))).astype(np.float32)
    return dict(ids=ids, frames=frames, local_pose=local, global_pose=glob, pred_cam_t=cam_t, focal_length=focal, shape=shape)


def _vis(case, dev, rows=slice(None)):
    """a vis_dict of the case's rows on the device (the camera outputs are placeholders that have to pass through)"""
    d = {k: torch.from_numpy(case[k][rows]).to(dev) for k in ('local_pose', 'global_pose', 'pred_cam_t', 'focal_length', 'shape')}
    n = d['shape'].shape[0]
    d['cam_rotmat'] = torch.eye(3, device=dev).repeat(n, 1, 1)
    d['render_rotmat'] = torch.eye(3, device=dev).repeat(n, 1, 1) * 2
    d['local_smpl_vertices'] = torch.zeros(n, 6890, 3, device=dev)
    d['smpl_vertices'] = torch.zeros(n, 6890, 3, device=dev)
    return d


@pytest.fixture(scope='module')
def tracks(dev, model):
    """the 12-row case, smoothed in one call on the device, with the restatement in float64 and float32 -- computed once, shared, never changed"""
    from whmr_amd.demo import TrackSmoother
    case = _tracks_case()
    sm = TrackSmoother(model, **PARAMS)
    vis = _vis(case, dev)
    out = sm.smooth(vis, case['ids'], case['frames'])
    args = [case[k] for k in ('local_pose', 'global_pose', 'pred_cam_t', 'focal_length', 'shape')] + [case['ids'], case['frames']]
    ref = {dt: SR.smooth_tracks(*args, dtype=dt, **PARAMS) for dt in (np.float64, np.float32)}
    return dict(case=case, vis=vis, out=out, rotmats=sm.rotmats, state=[s.clone() for s in sm._state], ref=ref, sm=sm)


def _figures(local_rotmat, global_rotmat, local_pose, global_pose, cam_t, focal, shape):
    """the compared quantities as float64 arrays; poses enter as ROTATIONS (the sign of an angle-axis vector at pi is free)"""
    f = lambda a: np.asarray(a, dtype=np.float64)
    P = f(shape).shape[0]
    return dict(local_rotmat=f(local_rotmat), global_rotmat=f(global_rotmat), local_pose=SR.rot_exp(f(local_pose).reshape(P, 24, 3)),
                global_pose=SR.rot_exp(f(global_pose).reshape(P, 24, 3)), cam_t=f(cam_t), focal=f(focal), shape=f(shape))


def _ref_figures(ref):
    """the restatement's outputs in the same form; its poses are log of its rotations, rounded to its dtype"""
    dt = ref['shape'].dtype.type
    return _figures(ref['local_rotmat'], ref['global_rotmat'], SR.rot_log(ref['local_rotmat'], dt), SR.rot_log(ref['global_rotmat'], dt), ref['cam_t'],
                    ref['focal'], ref['shape'])


def test_kernel_equals_the_float64_reference(tracks):
    """every compared quantity within 4 x the float32 restatement's own distance from float64 (1.05e-6 on these inputs, see the header); the figures of
    both are printed before anything is asserted"""
    case, out = tracks['case'], tracks['out']
    want, want32 = _ref_figures(tracks['ref'][np.float64]), _ref_figures(tracks['ref'][np.float32])
    own = {k: ew_err(want32[k], want[k]) for k in want}
    gate = 4 * max(own.values())
    c = lambda t: t.cpu().numpy()
    got = _figures(c(tracks['rotmats'][0]), c(tracks['rotmats'][1]), c(out['local_pose']), c(out['global_pose']), c(out['pred_cam_t']),
                   c(out['focal_length']), c(out['shape']))
    errs = {k: ew_err(got[k], want[k]) for k in want}
    for k in want:
        print('%-14s float32 restatement %.2e   device %.2e' % (k, own[k], errs[k]))
    print('gate = 4 x %.2e = %.2e' % (max(own.values()), gate))
    assert 0 < gate <= GATE
    for k, e in errs.items():
        assert e <= gate, (k, e, gate)
    # every branch ran: the static joint barely moved, the step joint is on its way, the root sits at pi
    R64 = tracks['ref'][np.float64]['local_rotmat']
    a_rows = [r for r, i in enumerate(case['ids']) if i == 'a']
    assert np.linalg.norm(SR.rot_log(R64[a_rows[-1], 5].T @ R64[a_rows[0], 5])) < 1e-3
    assert 0.5 < np.linalg.norm(SR.rot_log(R64[a_rows[1], 7].T @ R64[a_rows[-1], 7])) < 3.0
    assert (np.linalg.norm(SR.rot_log(R64[:, 0]), axis=-1) > np.pi - 0.05).all()
    # the single-sample track and the untracked row come back bit for bit; the camera outputs pass through
    for r in (case['ids'].index('c'), case['ids'].index(None)):
        for k in ('local_pose', 'global_pose', 'pred_cam_t', 'focal_length', 'shape'):
            assert torch.equal(out[k][r], tracks['vis'][k][r]), (r, k)
    assert set(out) == set(tracks['vis'])
    for k in ('cam_rotmat', 'render_rotmat'):
        assert out[k] is tracks['vis'][k]
    # and a filtered row is not its input
    assert not torch.equal(out['pred_cam_t'][a_rows[-1]], tracks['vis']['pred_cam_t'][a_rows[-1]])
    # a second smoother on the same inputs: bit-identical
    from whmr_amd.demo import TrackSmoother
    sm2 = TrackSmoother(tracks['sm'].model, **PARAMS)
    again = sm2.smooth(tracks['vis'], case['ids'], case['frames'])
    for k in KEYS:
        assert torch.equal(again[k], out[k]), k


def test_streamed_long_track_stays_orthonormal(dev, model):
    from scipy.spatial.transform import Rotation
    from whmr_amd.demo import TrackSmoother
    rng = np.random.default_rng(5)
    n, chunk = 512, 64
    walk = np.cumsum(rng.normal(0, 0.25, size=(n, 25, 3)), 0)                        # large motion: every step rotates by a good fraction of a radian
    pose = Rotation.from_rotvec(walk.reshape(-1, 3)).as_rotvec().reshape(n, 25, 3).astype(np.float32)
    case = dict(local_pose=pose[:, :24].reshape(n, 72), global_pose=np.concatenate([pose[:, 24], pose[:, 1:24].reshape(n, 69)], 1),
                pred_cam_t=rng.normal(0, 1, size=(n, 3)).astype(np.float32), focal_length=rng.uniform(500, 1500, size=n).astype(np.float32),
                shape=rng.normal(0, 1, size=(n, 10)).astype(np.float32))
    sm = TrackSmoother(model, max_tracks=1, **PARAMS)
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    worst = torch.zeros((), dtype=torch.float64, device=dev)
    for s in range(0, n, chunk):
        sm.smooth(_vis(case, dev, slice(s, s + chunk)), ['t'] * chunk, range(s, s + chunk))
        for R in sm.rotmats:
            R = R.double()
            worst = torch.maximum(worst, (R.transpose(-1, -2) @ R - eye).abs().max())
    print('max |R^T R - I| over 512 streamed samples: %.2e' % worst.item())
    assert worst.item() <= 1e-5
    assert (torch.linalg.det(sm._state[0].double().view(-1, 3, 3)) > 0.99).all()


def test_streaming_equals_one_call(dev, model, tracks):
    from whmr_amd.demo import TrackSmoother
    case = tracks['case']
    sm = TrackSmoother(model, **PARAMS)
    parts, rot = [], []
    for rows in (slice(0, 4), slice(4, 12)):                                        # frames 0-1, then frames 2-5
        parts.append(sm.smooth(_vis(case, dev, rows), case['ids'][rows], case['frames'][rows]))
        rot.append(sm.rotmats)
    for k in KEYS:
        assert torch.equal(torch.cat([p[k] for p in parts]), tracks['out'][k]), k
    for j in (0, 1):
        assert torch.equal(torch.cat([r[j] for r in rot]), tracks['rotmats'][j])
    assert sm._slots == tracks['sm']._slots and sm._last == tracks['sm']._last
    for a, b in zip(sm._state, tracks['state']):
        assert torch.equal(a[:3], b[:3])
    assert tracks['state'][0][:3].abs().sum() > 0


def test_vertices_are_the_smpl_of_the_returned_pose_and_shape(model, tracks):
    out, (local_R, global_R) = tracks['out'], tracks['rotmats']
    smpl = model.regressor[0].smpl
    assert torch.equal(out['local_smpl_vertices'], smpl.run(out['shape'], local_R).vertices)
    assert torch.equal(out['smpl_vertices'], smpl.run(out['shape'], global_R).vertices)
    assert torch.equal(global_R[:, 1:], local_R[:, 1:]) and torch.equal(out['global_pose'][:, 3:], out['local_pose'][:, 3:])
    assert out['local_smpl_vertices'].abs().max() > 0.1


# ----------------------------------------------------------------------------- the stage behind the model
IDS = [['p', 'q'], ['q', 'p'], ['p', 'q'], ['p', 'q']]                              # the tracker's ids: the two persons swap rows in frame 1
FLAT_IDS, FLAT_FRAMES = [i for f in IDS for i in f], [0, 0, 1, 1, 2, 2, 3, 3]


@pytest.fixture(scope='module')
def clip(dev, model):
    """a 4-frame, 2-person synthetic clip and its unsmoothed result (person batch padded to 4, as the pipeline below pads it)"""
    from whmr_amd.demo import infer_clip
    rng = np.random.default_rng(9)
    frames = torch.from_numpy(rng.integers(0, 256, size=(4, 90, 120, 3), dtype=np.uint8)).to(dev)
    c = rng.uniform(-4, 4, size=(4, 2, 2))
    dets = [[(45.0 + c[f, 0, 0], 40.0 + c[f, 0, 1], 60.0, 60.0), (85.0 + c[f, 1, 0], 45.0 + c[f, 1, 1], 50.0, 50.0)] for f in range(4)]
    dets[1] = dets[1][::-1]
    return frames, dets, infer_clip(model, frames, dets, pad_to=4)


def test_limits_of_the_filter(model, clip):
    from whmr_amd.demo import TrackSmoother
    _, _, plain = clip
    follow = TrackSmoother(model, min_cutoff=1e9).smooth(plain, FLAT_IDS, FLAT_FRAMES)     # a cut-off far above the frame rate: the input comes back
    assert set(follow) == set(plain)
    for k in plain:
        e = ew_err(follow[k], plain[k])
        print('follow %-22s ew_err %.2e' % (k, e))
        assert e < GATE, (k, e)
    sm = TrackSmoother(model, min_cutoff=1e-9, beta=0.0)                                     # no cut-off at all: every row holds its track's first sample
    hold = sm.smooth(plain, FLAT_IDS, FLAT_FRAMES)
    first = torch.tensor([FLAT_IDS.index(i) for i in FLAT_IDS], device=plain['shape'].device)
    for k in KEYS:
        if k in ('local_pose', 'global_pose'):
            continue                                                                 # compared as rotations below
        e = ew_err(hold[k], plain[k][first])
        print('hold   %-22s ew_err %.2e' % (k, e))
        assert e < GATE, (k, e)
    for R in sm.rotmats:
        e = ew_err(R, R[first])
        assert e < GATE, e
    assert ew_err(hold['local_smpl_vertices'], plain['local_smpl_vertices']) > GATE         # the clip does move


def test_pipeline_smooths_behind_the_graph_and_draws_it(model, clip):
    import mesh_render_reference as MR
    from whmr_amd.demo import ClipPipeline, TrackSmoother, infer_clip, render_frame
    from whmr_amd.utils.renderer_cam import MeshRenderer
    frames, dets, plain = clip
    r = MeshRenderer(MR.uv_sphere()[1])
    pipe = ClipPipeline(model, person_bucket=4, renderer=r, smoother=TrackSmoother(model, **PARAMS))
    out, images = pipe(frames, dets, track_ids=IDS)
    fresh = TrackSmoother(model, **PARAMS)
    eager = infer_clip(model, frames, dets, pad_to=4, track_ids=IDS, smoother=fresh)
    assert set(out) == set(eager) == set(plain) and pipe.smoother.frame_counter == fresh.frame_counter == 4
    for k in eager:
        assert torch.equal(out[k], eager[k]), k
    assert out['frame_index'].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    assert not torch.equal(out['pred_cam_t'][6:], plain['pred_cam_t'][6:])
    # the renderer drew the smoothed rows: frame 3's picture is the smoothed rows' picture, and not the unsmoothed one
    rows = lambda d: {k: d[k][6:8] for k in ('local_smpl_vertices', 'pred_cam_t', 'focal_length')}
    assert torch.equal(images[3], render_frame(rows(out), frames[3], r))
    assert not torch.equal(images[3], render_frame(rows(plain), frames[3], r))
    # without track ids the same pipeline is today's: the replayed result bit for bit, the unsmoothed picture, no time passes for the smoother
    out2, images2 = pipe(frames, dets)
    for k in plain:
        assert torch.equal(out2[k], plain[k]), k
    assert torch.equal(images2[3], render_frame(rows(plain), frames[3], r)) and pipe.smoother.frame_counter == 4 and len(pipe._graphs) == 1
